// hm_stats_pairs_dev.h - the device functions of the pair arithmetic that the all-pairs statistics on float64 frames (hm_stats.hip:
// k_pair_stats, k_pairs_stats, k_pairs_stats_lds) and on DN frames (hm_stats_dn.hip) share: the difference terms of one element, a wave's
// iteration over its chunks (whole: pair_process_any; partial: pair_tail_with). Where an operand comes from -
// a float64 frame, an LDS stage, a per-DN table - is the caller's business: the arithmetic, the fold points and the element order are
// here, once, so that every kernel built on them gives the same bits for the same operand values. At the end: the read of one entry of
// the per-DN table, shared by the units that read DN frames (hm_stats_dn.hip, hm_stats_hist_dn.hip).
#pragma once
#include "hm_moments.h"

namespace hm {

// ---- pair-fused linearity statistics ----------------------------------------------------------
// ExposurePair.compute_difference + compute_stats(axis=(0,1)) (modules/exposure_series.py:33-54, called per pair
// by process_linearity :443-446) without materialising the two difference images and in one pass: x, y (and their stds) are read
// once and both the absolute and the relative difference are reduced. out: 6*C doubles
// [abs mean | abs std | abs error | rel mean | rel std | rel error].
// difference terms of one element (measurand.py:634-653) and the statistics weights 1 / std of both differences. One reciprocal
// (1 / scale) and two reciprocal square roots per element: x / (m y) = x r, (ys x) / (m y^2) = ys x m r^2 with r = 1 / (m y), and
// w = 1 / sqrt(q), std = q w - a few ulp from the reference's three divisions, two square roots and two reciprocals (the pair
// kernels are FP64-VALU bound); the statistics agree with the oracle to 1e-12.
// GUARD = false leaves out the selects that keep the hardware estimate where it is 0 or infinite (scale, q = 0 or inf) and reports in
// `special` whether this lane had such an estimate: the caller redoes the element with GUARD = true when any lane of the wave did
// (wave-uniform branch; both forms give the same bits everywhere else, NaNs propagate through the Newton steps by themselves).
constexpr int kClassZeroInf = 0x264;                    // v_cmp_class_f64 mask: -inf | -0 | +0 | +inf
template <bool STD, bool GUARD>
__device__ __forceinline__ void pair_terms(double xv, double xs, double yv, double ys, double mult,
                                           double& a, double& as, double& wa, double& r, double& rs, double& wr, bool& special) {
    const double scale = mult * yv;                     // measurand.py:634
    a = xv - scale;                                     // :635
    double inv;
    if constexpr (GUARD) inv = rcp_nr(scale);
    else {
        const double r0 = __builtin_amdgcn_rcp(scale);
        inv = rcp_newton<HM_PAIR_NEWTON>(scale, r0);
        special = __builtin_amdgcn_class(r0, kClassZeroInf);
    }
    r = a * inv;                                        // :636
    wa = 1.0; wr = 1.0;
    if constexpr (STD) {
        const double m1 = mult * ys;
        const double qa = xs * xs + m1 * m1;            // :652
        const double u1 = xs * inv;
        const double u2 = ((ys * xv) * mult) * (inv * inv);
        const double qr = u1 * u1 + u2 * u2;            // :653
        if constexpr (GUARD) {
            wa = rsqrt_nr(qa, as);
            wr = rsqrt_nr(qr, rs);
        } else {
            const double ya0 = __builtin_amdgcn_rsq(qa), yr0 = __builtin_amdgcn_rsq(qr);
            wa = rsq_newton<HM_PAIR_NEWTON>(qa, ya0); as = qa * wa;
            wr = rsq_newton<HM_PAIR_NEWTON>(qr, yr0); rs = qr * wr;
            special = special || __builtin_amdgcn_class(ya0, kClassZeroInf) || __builtin_amdgcn_class(yr0, kClassZeroInf);
        }
    }
}

// The element loop of the pair kernels for ONE wave: chunks of 64 consecutive elements starting at sb0, sb0 + stride, ... (sb0 and
// stride wave-uniform, stride a multiple of C so that a lane's elements share a channel). Whole chunks take the select-free path;
// the last, partial ones hand their missing elements to the accumulators as NaNs. Both Welford states fold every kMomBlock elements.
// SX / SY: the first / second operand has a std image (compile-time, so that no load sits behind a branch: the waits in front of an
// iteration's arithmetic can then leave the NEXT iteration's loads in flight); statistics are weighted when either has one.
constexpr int kPairUN = 2;                     // 64-element chunks per wave iteration (sb and sb + stride)
template <bool STD, int UN = kPairUN, bool LEAN = false>
__device__ __forceinline__ void pair_process(MomAcc (&st)[2], int it, double mult, const double (&xv)[UN], const double (&xs)[UN],
                                             const double (&yv)[UN], const double (&ys)[UN]) {
#pragma unroll
    for (int u = 0; u < UN; ++u) {
        double av, as = 0.0, wa, rv, rs = 0.0, wr;
        bool special = false;
        pair_terms<STD, false>(xv[u], xs[u], yv[u], ys[u], mult, av, as, wa, rv, rs, wr, special);
        if (__builtin_amdgcn_ballot_w64(special) != 0)                           // a zero / infinite scale or variance somewhere in the wave
            pair_terms<STD, true>(xv[u], xs[u], yv[u], ys[u], mult, av, as, wa, rv, rs, wr, special);
        acc_add_pair<STD, LEAN>(st[0], av, wa, as);
        acc_add_pair<STD, LEAN>(st[1], rv, wr, rs);
    }
    // every kMomBlock elements, whatever UN; weighted: + the early fold (unweighted an outlier counts in full and sets the scale of the
    // variance itself - and the extra condition cost the unweighted all-pairs kernel 3.5 %: 1 160 -> 1 203 us)
    if ((it & (kMomBlock / UN - 1)) == kMomBlock / UN - 1 || (STD && it == 0)) { acc_fold<true>(st[0]); acc_fold<true>(st[1]); }
}

// whole chunks only (all 64 lanes active): the lean body once every lane of the wave has seen a valid element of both differences
// (normally from the first iteration on) - 8 of ~106 VALU instructions per two element-pairs less in a kernel that is VALU-bound
#ifndef HM_PAIR_LEAN
#define HM_PAIR_LEAN 1
#endif
template <bool STD, int UN = kPairUN>
__device__ __forceinline__ void pair_process_any(MomAcc (&st)[2], int it, double mult, const double (&xv)[UN], const double (&xs)[UN],
                                                 const double (&yv)[UN], const double (&ys)[UN]) {
    // (without std only: with std the all-pairs kernel sits at the 128 VGPRs a 1024-thread workgroup may use and two bodies make it spill)
#ifndef HM_PAIR_LEAN_STD
#define HM_PAIR_LEAN_STD 0
#endif
    if constexpr (HM_PAIR_LEAN && (!STD || HM_PAIR_LEAN_STD)) {
        if (__builtin_amdgcn_ballot_w64(st[0].haveK && st[1].haveK) == ~0ull) { pair_process<STD, UN, true>(st, it, mult, xv, xs, yv, ys); return; }
    }
    pair_process<STD, UN, false>(st, it, mult, xv, xs, yv, ys);
}

// the wave's last, partial chunks (from iteration `it` at element sb on), then the final fold. operands(qc, ok, xv, xs, yv, ys) gives the
// four operands of element qc (xs, ys: 0.0 where there is no std); a lane whose element q is past the end asks for element n - 1 (a valid
// address) with ok = false, and operands() hands its element in as NaN: xv and, with stds, xs
template <bool STD, int UN, class Operands>
__device__ __forceinline__ void pair_tail_with(MomAcc (&st)[2], int it, int64_t sb, double mult, int64_t n, int64_t stride, uint32_t lane,
                                               Mom (&mine)[2], Operands operands) {
    for (; sb < n; sb += UN * stride, ++it) {
        double xv[UN], yv[UN], xs[UN], ys[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int64_t q = sb + u * stride + lane;
            const bool ok = q < n;
            const int64_t qc = ok ? q : n - 1;
            operands(qc, ok, xv[u], xs[u], yv[u], ys[u]);
        }
        pair_process<STD, UN>(st, it, mult, xv, xs, yv, ys);
    }
    mine[0] = acc_finish<true>(st[0], STD);
    mine[1] = acc_finish<true>(st[1], STD);
}

// ---- the per-DN table of the entries that read DN frames (hm_stats_dn.hip, hm_stats_hist_dn.hip) ----
typedef double f64x2 __attribute__((ext_vector_type(2)));

// entry `at` of a table at `tab` (global memory, or the LDS copy: the caller's pointer carries the address space)
template <bool STD, class P>
__device__ __forceinline__ void dn_entry(P tab, uint32_t at, double& v, double& s) {
    if constexpr (STD) {
        const f64x2 e = *reinterpret_cast<const f64x2*>(tab + at * 16u);
        v = e.x; s = e.y;
    } else {
        v = *reinterpret_cast<const double*>(tab + at * 8u);
        s = 0.0;
    }
}

}  // namespace hm
