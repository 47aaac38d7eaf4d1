// hm_stats_math.h - the element rules of the histograms, of the kernel density estimate and of the per-DN table of hm_pairs_statistics_dn, one text for the device units
// (hm_stats_hist.hip, hm_kde.hip) and ../csrc_host/hm_host.cpp. np.histogram with `bins` equal-width bins on [lo, hi] (compute_channel_histogram, modules/measurand.py:430-469): the bin of x is
// int((x - lo) * bins / (hi - lo)), corrected against the actual edges (np.linspace(lo, hi, bins + 1), passed in by the caller) exactly as
// numpy/lib/_histograms_impl.py does, the right edge inclusive. Non-finite values are skipped (:453); with weights, elements whose std is 0
// are skipped and the weight is 1 / std (:457-460).
//
// DEVICE / HOST - the builds perform the same operations here. The two index forms differ inside BOTH builds, on purpose:
//   hist_bin            hm_channel_histogram: int((x - lo) * norm), then `== bins -> bins - 1`; its edges are the caller's checked host array.
//   hist_bin_bounded    hm_pairs_histogram: the same index written so that no edge array can take it outside 0..bins-1 (on the device the
//                       edges are device data nobody has checked).
#pragma once
#include "hm_math_common.h"

namespace hm {

HM_MATH_FN bool hist_finite(double x) { return fabs(x) <= 1.79769313486231570e308; }                 // isfinite
// weight 1 / std of an element with a std; false: std == 0, the element is not counted (measurand.py:457, :460)
HM_MATH_FN bool hist_weight(double s, double& w) { if (s == 0.0) return false; w = 1.0 / s; return true; }
HM_MATH_FN bool hist_in_range(double x, double lo, double hi) { return x >= lo && x <= hi; }         // outside the range: not counted

// the two corrections of a computed index against the actual edges: left-closed bins, the last one closed on the right too
HM_MATH_FN int hist_bin_adjust(int idx, double x, const double* edges, int bins) {
    if (x < edges[idx]) idx -= 1;
    else if (x >= edges[idx + 1] && idx != bins - 1) idx += 1;
    return idx;
}
// bin of a value inside [lo, hi], norm = bins / (hi - lo)
HM_MATH_FN int hist_bin(double x, double lo, double norm, const double* edges, int bins) {
    int idx = static_cast<int>((x - lo) * norm);
    if (idx == bins) idx -= 1;
    return hist_bin_adjust(idx, x, edges, bins);
}
// x >= lo = edges[0] rules out the step below bin 0, the step up is not taken from the last bin
HM_MATH_FN int hist_bin_bounded(double x, double lo, double norm, const double* edges, int bins) {
    const double t = (x - lo) * norm;
    const int idx = t < static_cast<double>(bins) ? static_cast<int>(t) : bins - 1;
    return hist_bin_adjust(idx, x, edges, bins);
}

// counted element e of a kernel density estimate: finite x, and std != 0 when std is given; w = 1 / std or 1
HM_MATH_FN bool kde_load(const double* __restrict__ val, const double* __restrict__ std_, int64_t e, double& x, double& w) {
    x = val[e];
    w = 1.0;
    bool ok = isfinite(x);
    if (std_) { const double s = std_[e]; ok = ok && s != 0.0; w = 1.0 / s; }
    return ok;
}

// hm_pairs_statistics_dn: the thresholded table entry at = idx * C + c of a DN frame. apply_thresholds (modules/measurand.py:375-428) decides
// on the value for the value and its std (a NaN compares false and stays); the std is measurand.py:512 on calculate_numerical_STD's std
HM_MATH_FN void pairs_dn_entry(const double* icrf, const double* icrf_diff, const double* std_table, int64_t at, double lo, double hi,
                               double& v, double& s) {
    v = icrf[at];
    s = std_table ? icrf_diff[at] * std_table[at] : 0.0;
    if (v < lo || v > hi) {
        v = __builtin_nan("");
        if (std_table) s = __builtin_nan("");
    }
}

}  // namespace hm
