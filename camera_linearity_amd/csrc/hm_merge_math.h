// hm_merge_math.h - the element formulas of linearize and the fused merge, one text for the device units and ../csrc_host/hm_host.cpp:
// the Gaussian weight and its derivative, the index linearize forms from a float64 value, the 'reflect' index fold of the k x k medians,
// the flat-field epilogue and the variance term of one frame. Loads, stores, tables and loop structure stay with their kernels.
//
// DEVICE / HOST - where the two builds perform different operations, on purpose; no output bit of either build moves here:
//   lut_index           the host build returns 0 for NaN and beyond +-9.2e18 (the cast of such a double to an integer is undefined there);
//                       the device build casts as it stands.
//   flat_field_math     1 / F**2 formed once and multiplied: every merge kernel, the host merge and the HOST build's hm_normalize_by_map.
//   flat_field_exact    the reference's own divisions, operation for operation: the DEVICE build's hm_normalize_by_map only.
//   gauss_weight        HM_FAKE_EXP (a timing experiment of the device build) replaces exp(); never defined for the host build.
#pragma once
#include "hm_math_common.h"

namespace hm {

// Gaussian weight of the merge, measurand.py:615: w = e ** (-30 (v - 0.5)^2) with dv = v - 0.5, wherever it is evaluated analytically
#ifdef HM_FAKE_EXP          /* timing experiment only: removes the cost of exp() */
HM_MATH_FN double gauss_weight(double dv) { return 1.0 + -30.0 * (dv * dv); }
#else
HM_MATH_FN double gauss_weight(double dv) { return exp(-30.0 * (dv * dv)); }
#endif
// its derivative from the weight, measurand.py:616: -2 * 30 * (v - 0.5) * w
HM_MATH_FN double gauss_dweight(double dv, double w) { return (-60.0 * dv) * w; }

// index linearize forms from a float64 value, measurand.py:503: around(v * 255) (half to even), astype(uint8) - wraps modulo 256
HM_MATH_FN uint32_t lut_index(double v) {
    const double r = rint(v * 255.0);
#ifndef __HIP_DEVICE_COMPILE__
    if (!(r == r) || r >= 9.2e18 || r <= -9.2e18) return 0u;
#endif
    return static_cast<uint32_t>(static_cast<int64_t>(r)) & 255u;
}

// scipy.ndimage 'reflect' (d c b a | a b c d) index fold, valid for any offset
HM_MATH_FN int64_t reflect_index(int64_t i, int64_t n) {
    while (i < 0 || i >= n) {
        if (i < 0) i = -i - 1;
        if (i >= n) i = 2 * n - i - 1;
    }
    return i;
}

// flat-field epilogue on loaded operands, modules/measurand.py:585-602. The value keeps the reference's operations, (val / F) * m (:602).
// The three variance terms (:586-596) each divide by F**2 or F**4 in the reference; here the caller forms iF2 = 1 / (F * F) once (1.0
// without std) and it is multiplied (3 float64 divisions fewer per element; the std moves by <= 2 ulp, its test tolerance is 1e-9).
HM_MATH_FN void flat_field_math(double F, double iF2, double sF, double m, double s, bool with_std, double& val, double& sd) {
    if (with_std) {
        const double v2 = val * val;
        const double u_acq = ((sd * sd) * iF2) * (m * m);
        const double u_ff = ((v2 * (iF2 * iF2)) * (sF * sF)) * (m * m);
        const double u_ffm = (v2 * iF2) * (s * s);
        sd = sqrt(u_acq + u_ff + u_ffm);
    }
    val = (val / F) * m;
}

// the same epilogue operation for operation as the reference writes it (measurand.py:585-602)
HM_MATH_FN void flat_field_exact(double v, double s0, double F, double sF, double m, double s, bool with_std, double& ov, double& os) {
    if (with_std) {
        const double F2 = F * F;
        double u_acq = (s0 * s0) / F2;        // measurand.py:586-587
        u_acq *= m * m;
        double u_ff = (v * v) / (F2 * F2);    // :590-592
        u_ff *= sF * sF;
        u_ff *= m * m;
        double u_ffm = (v * v) / F2;          // :595-596
        u_ffm *= s * s;
        os = sqrt(u_acq + u_ff + u_ffm);      // :599
    }
    ov = (v / F) * m;                         // :602
}

// variance term of one frame, exposure_series.py:389: weight w and its derivative dw, linearized value g and its uncertainty dg
// (measurand.py:512), invS = 1 / S and invS2 = 1 / S**2 of the element (:343), it = 1 / exposure. The caller accumulates term * term.
HM_MATH_FN double merge_var_term(double w, double dw, double g, double dg, double invS, double invS2, double it) {
    const double A = (dw * g + w * dg) * invS - ((dw * w) * g) * invS2;
    return (A * dg) * it;
}

}  // namespace hm
