// hm_moments.h - what every reduction of the statistics units (hm_stats.hip, hm_stats_axis.hip) shares on the device: the one-pass moment
// states (Mom, MomAcc) with their fold / merge / finish, the workgroup and grid combinations, the Newton reciprocals of the FP64-bound pair
// kernels, and the grid of the reductions (kStatBlocks, stat_grid). No kernel, no entry point.
#pragma once
#include "hm_common.h"

namespace hm {

// ---- statistics -------------------------------------------------------------------------------
// compute_dimension_statistics (modules/measurand.py:318-350) in ONE pass over the data. The reference's two NumPy passes
// (mean, then sum of squared deviations from it) would read every byte twice; here every thread keeps a running (W, mean, M2)
// of its elements (short blocks of shifted sums folded in with Chan's formula, see MomAcc) and thread, wave, workgroup and grid
// partials are combined with the same pairwise formula in a fixed tree order (bit-reproducible; as stable as the two-pass form:
// moments are always taken about a mean of the data they cover). NaNs are skipped exactly as np.nansum / np.nanmean do, term by
// term: `Wall` sums every non-NaN weight (the reference's denominators), the moments take the elements whose v * w is FINITE.
// Infinite terms (a relative difference against y = 0 is one) never enter the moments - inf - K would poison them with NaN where NumPy
// still answers: their SUM (+inf, -inf, or NaN when both signs occurred) is added into M2, which has no other meaning once a term was
// infinite, survives every fold and merge there (inf + finite = inf), and mom_finish() then gives NumPy's answers (mean = +-inf / NaN by sign,
// nanstd = NaN; the weighted formulas' inf or 0) - see there.
// workgroups of the reduction kernels: 3 per CU. A/B on one box (tools/ab_ops.sh, tools/ab_lin.sh, profiles/r02h_ab_stat_blocks.log): 2040
// -> 768 takes channel statistics from 0.65 / 0.59 to 0.73 / 0.69 of 8 TB/s and the all-pairs kernel from 1.53 / 2.91 to 1.37 / 2.77 ms
#ifndef HM_STAT_BLOCKS
#define HM_STAT_BLOCKS 768
#endif
constexpr int kStatBlocks = HM_STAT_BLOCKS;                           // a multiple of 12: total threads divisible by C = 1..4

// per = elements per workgroup and trip: 256 (a thread each: channel and pair statistics) or 64 (a wave row: the all-pairs statistics)
inline int stat_grid(int64_t n, int per) {
    int64_t g = (n + per - 1) / per;
    g = ((g + 11) / 12) * 12;
    return static_cast<int>(g < kStatBlocks ? g : kStatBlocks);
}

struct Mom {
    double Wall;        // sum of the non-NaN weights (unweighted: count of non-NaN values)
    double W;           // weight of the elements in (mean, M2)
    double mean, M2;    // weighted mean and sum of w (v - mean)^2 of those elements
    double ss, cs;      // sum and count of the non-NaN stds (`error` = nanmean(std)); unused without std
};
constexpr int kMomVals = 6;
__device__ __forceinline__ Mom mom_zero() { return Mom{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// Per-thread accumulation, branch-free: kMomBlock (64) elements are summed as shifted moments about K = the state's current mean
// (S0 = sum w, S1 = sum w (v - K), S2 = sum w (v - K)^2: three FMAs per element, no division), an element that NumPy's nan-functions
// would skip enters with weight 0 and deviation 0 (selects, no branch), and the block is folded into the running (W, mean, M2) with
// Chan's formula when the LOOP COUNTER says so (wave-uniform) - two divisions per block instead of two per element. K tracks the data
// (until the first fold it is the first valid element), so S2 - S1^2 / S0 differences nothing large. The FIRST fold comes early - after a
// lane's first iteration (2-4 elements) - because that first element may be an outlier that barely counts (a relative difference against
// y ~ 0 with its huge std: weight ~ 0): as the shift of a whole 64-element block it cost eps (K - mean)^2 / sigma^2 = 1e-7 on the std
// (tools/fuzz_backends.py --scale 6); after two elements the weighted mean is already the ordinary one.
#ifndef HM_MOM_BLOCK
#define HM_MOM_BLOCK 64      // round 4: 8 -> 64. A fold is two reciprocals, a dozen multiplies and a branch per state; the all-pairs kernel (FP64-VALU
#endif                       // bound, two states per wave) went 2 673 -> 2 440 us with std and 1 429 -> 1 210 us without on one box (16: 2 548 / 1 305,
                             // 32: 2 485 / 1 245, 128: 2 425 / 1 190, 256: 2 407 / 1 260; tools/gpu_r04d.sh, profiles/r04d_*). K is refreshed with the
                             // running mean at every fold and starts as a data element, so 64 shifted terms difference nothing large.
constexpr int kMomBlock = HM_MOM_BLOCK;
struct MomAcc {
    Mom m;
    double K, S0, S1, S2;
    bool haveK;
    int cnt;            // acc_add_pair: count of the non-NaN stds as an integer (folded into m.cs by acc_finish)
};
__device__ __forceinline__ MomAcc acc_zero() { return MomAcc{mom_zero(), 0.0, 0.0, 0.0, 0.0, false, 0}; }
// the shift K of a block must be finite (inf - K has to keep its sign): an infinite first element gives +-1e300, and the block it poisons
// (S1 = +-inf / NaN) is then set aside by acc_fold()
__device__ __forceinline__ double finite_shift(double v) { return fmin(fmax(v, -1e300), 1e300); }
__device__ __forceinline__ bool is_finite(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000ll); }   // false for NaN and +-inf

// 1 / x and 1 / sqrt(q) to within ~1 ulp without the IEEE expansions and without branches: the hardware estimate (v_rcp_f64 /
// v_rsq_f64, about 26 bits; already the IEEE answer for 0, infinities and NaN) and two Newton steps, kept only when the estimate is a
// finite non-zero number - 7 / 10 instructions instead of 11 (divide) / ~26 (sqrt + divide).
__device__ __forceinline__ bool finite_nonzero(double x) { const double ax = fabs(x); return ax > 0.0 && ax < __builtin_huge_val(); }
// STEPS == 2 (the default) is ONE higher-order step from the 2^-24 hardware estimate instead of two Newton steps - the same or better
// accuracy in fewer instructions (checked on 2 M operands against long-double references: reciprocal 1 + e + e^2, e = 1 - x r0: 3 instead
// of 4 instructions, max 1.00 ulp either way; reciprocal square root y0 (1 + e/2 + 3 e^2 / 8), e = 1 - q y0^2: 5 instead of 7 instructions,
// max 1.25 ulp against 2.19 ulp). Round 3: -5 of 104 VALU instructions per element-pair of the weighted pair statistics.
template <int STEPS = 2>
__device__ __forceinline__ double rcp_newton(double x, double r0) {
    const double e = fma(-x, r0, 1.0);
    if constexpr (STEPS == 1) return fma(e, r0, r0);
    return fma(r0, fma(e, e, e), r0);
}
template <int STEPS = 2>
__device__ __forceinline__ double rsq_newton(double q, double y0) {
    if constexpr (STEPS == 1) {
        const double h = 0.5 * q;
        return y0 * fma(-h * y0, y0, 1.5);
    }
    const double e = fma(-(q * y0), y0, 1.0);
    return fma(y0, fma(0.375, e, 0.5) * e, y0);
}
#ifndef HM_PAIR_NEWTON
#define HM_PAIR_NEWTON 2
#endif
__device__ __forceinline__ double rcp_nr(double x) {
    const double r0 = __builtin_amdgcn_rcp(x);
    const double r = rcp_newton(x, r0);
    return finite_nonzero(r0) ? r : r0;
}
__device__ __forceinline__ double rsqrt_nr(double q, double& root) {       // also sqrt(q) = q * rsqrt(q)
    const double y0 = __builtin_amdgcn_rsq(q);
    const double y = rsq_newton(q, y0);
    const bool ok = finite_nonzero(y0);
    root = ok ? q * y : q;                                                   // sqrt(0) = 0, sqrt(inf) = inf, NaN stays NaN (q is a sum of squares)
    return ok ? y : y0;
}

// RCP: the two quotients of a fold as products with rcp_nr() (~1 ulp; 14 instructions instead of two IEEE division expansions) - the
// pair kernels, which are FP64-VALU bound and fold two states per 8 element-pairs
template <bool RCP = false>
__device__ __forceinline__ void acc_fold(MomAcc& a) {
    if (!a.haveK && a.S0 != 0.0) { a.K = a.S2; a.S2 = 0.0; }        // a lone parked element (weighted_first below): it is its own shift, d = 0
    if (!is_finite(a.S1)) {                                         // acc_add_pair let infinite terms in: their sum's class goes to M2, the block is not folded
        a.m.M2 += a.S1;
        a.K = 0.0; a.haveK = false;                                 // (K may be the clamped +-1e300 of an infinite first element: take a new one)
    } else if (a.S0 != 0.0) {                                       // (a lane whose whole block was skipped: rare)
        const double q = RCP ? a.S1 * rcp_nr(a.S0) : a.S1 / a.S0;   // block mean - K
        const double mb = a.K + q;
        const double M2b = a.S2 - a.S1 * q;
        if (a.m.W == 0.0) { a.m.W = a.S0; a.m.mean = mb; a.m.M2 += M2b; }      // (+= : M2 is 0 here - or already holds infinite terms)
        else {
            const double W = a.m.W + a.S0;
            const double d = mb - a.m.mean;
            const double f = RCP ? a.S0 * rcp_nr(W) : a.S0 / W;
            a.m.mean = a.m.mean + d * f;
            a.m.M2 = (a.m.M2 + M2b) + (d * d) * (a.m.W * f);
            a.m.W = W;
        }
        a.K = a.m.mean;
    }
    a.S0 = 0.0; a.S1 = 0.0; a.S2 = 0.0;
}

// WEIGHTED statistics, the first elements of a lane (no shift yet): the shift must not be an element that barely counts. A relative
// difference against y ~ 0 is huge AND has a huge std, i.e. a weight ~ 0: as the shift K of a block it makes every ordinary element
// contribute w (v - K)^2 ~ 1e14 to S2, and M2 = S2 - S1^2 / S0 then carries eps x that - 2.8e-6 on a std in one case of
// tools/fuzz_backends.py (seed 1760803113997506811: K = 1.4e6 with weight 4e-12 beside values of 0.05 with weight 54). So the first element
// is PARKED - its weight in S0, its value in S2, nothing accumulated - and when the second arrives the heavier of the two becomes K and both
// are accumulated about it (exactly: one of the two deviations is 0). Elements of weight 0 add nothing to the moments and are passed over.
// Returns true when the element has been dealt with here. (acc_fold turns a parked element that stayed alone into a block of its own.)
// Used by the HBM-bound kernels (acc_add: channel and axis statistics); the FP64-bound pair kernels keep the first element as the shift
// (see acc_add_pair) and with it the limit on unthresholded heavy-tailed data described in DESIGN.md 4.4.
__device__ __forceinline__ bool weighted_first(MomAcc& a, double v, double w) {
    if (w == 0.0) return true;
    if (a.S0 == 0.0) { a.S0 = w; a.S2 = v; return true; }          // park
    const double vp = a.S2, wp = a.S0;
    a.K = w > wp ? v : vp;
    const double dp = vp - a.K, dn = v - a.K;
    const double tp = wp * dp, tn = w * dn;
    a.S0 = wp + w; a.S1 = tp + tn; a.S2 = fma(tn, dn, tp * dp);
    a.haveK = true;
    return true;
}

// one element: value v, weight w (already formed; 1 when unweighted), std s for the `error` sum; in_range = the element exists (tail lanes)
__device__ __forceinline__ void acc_add(MomAcc& a, double v, double w, double s, bool weighted, bool in_range) {
    bool use;
    if (weighted) {
        const bool okw = in_range && (w == w);
        const bool oks = in_range && (s == s);
        a.m.Wall += okw ? w : 0.0;                                          // nansum(weights)
        a.m.ss += oks ? s : 0.0;                                            // nanmean(stds)
        a.m.cs += oks ? 1.0 : 0.0;
        const double vw = v * w;
        use = in_range && is_finite(vw);                                    // nansum(values * weights), nansum(weights * (values - mean)**2)
        a.m.M2 += (in_range && !use && vw == vw) ? vw : 0.0;                // an infinite term
    } else {
        use = in_range && is_finite(v);
        a.m.M2 += (in_range && !use && v == v) ? v : 0.0;
        w = 1.0;
    }
    if (weighted && use && !a.haveK) { weighted_first(a, v, w); return; }   // (rare: a lane's first two elements; v is finite here - v w is)
    // An element that outweighs everything the lane has seen so far by 2^10 (rare; a std of 1e-200 beside ordinary ones is the extreme) must
    // not sit in a block whose shift is somewhere else: its w (v - K)^2 would absorb the block's other terms in S2 to within u x the
    // weight ratio, and S2 - S1 q then cancels down to nothing. The block so far is folded and the element becomes the shift of a new one
    // (d = 0 exactly), as weighted_first() does for a lane's first two elements. Per lane; acc_fold() has no cross-lane step.
    if (weighted && use && fabs(w) > 0x1p10 * fabs(a.S0 + a.m.W)) { acc_fold<false>(a); a.K = v; }
    a.K = (!a.haveK && use) ? v : a.K;
    a.haveK = a.haveK || use;
    const double we = use ? w : 0.0;
    const double d = use ? v - a.K : 0.0;
    const double t = we * d;
    a.S0 += we; a.S1 += t; a.S2 = fma(t, d, a.S2);
}

template <bool RCP = false>
__device__ __forceinline__ Mom acc_finish(MomAcc& a, bool weighted) {
    acc_fold<RCP>(a);
    if (!weighted) a.m.Wall = a.m.W;
    a.m.cs += static_cast<double>(a.cnt);
    return a.m;
}

// acc_add for the pair kernels. Weighted: w = 1 / sqrt(q) >= 0 and s = sqrt(q) >= 0 are NaN together (q NaN), so max(., 0) replaces
// the NaN selects of nansum(weights) / nansum(stds) and ONE comparison counts the non-NaN stds in an integer. Unweighted: w = 1.
// Elements that do not exist (tail lanes) must arrive as NaNs (value, and std when weighted).
// max(x, 0) with NaN -> 0 as ONE v_max_f64: fmax() puts a canonicalising v_max_f64 x, x in front because it cannot rule out a
// signalling NaN; x is the result of arithmetic here, never one
__device__ __forceinline__ double max0_nan_to_zero(double x) {
    double r;
    asm("v_max_f64 %0, %1, 0" : "=v"(r) : "v"(x));
    return r;
}
// LEAN: every lane of the wave already has its shift K (haveK set), so the two selects that look for the first valid element are
// dead - the caller checks that with one ballot per iteration (pair_process_any). Same bits either way.
#ifndef HM_PAIR_EXEC
#define HM_PAIR_EXEC 1       // round 4: all-pairs statistics 2 456-2 469 -> 2 337-2 341 us with std, 1 208-1 213 -> 1 154-1 161 us without (one box,
#endif                       // two runs each, profiles/r04k_pair_exec_ab.log); 0 = the select form
template <bool WEIGHTED, bool LEAN = false>
__device__ __forceinline__ void acc_add_pair(MomAcc& a, double v, double w, double s) {
    bool use;
    if constexpr (WEIGHTED) {
        a.m.Wall += max0_nan_to_zero(w);
        a.m.ss += max0_nan_to_zero(s);
        a.cnt += (s == s) ? 1 : 0;
        const double vw = v * w;
        use = vw == vw;
    } else {
        use = v == v;
    }
    // Infinite terms (unweighted: a relative difference against y = 0) are NOT filtered per element here - these kernels are FP64-issue
    // bound and a second branch per state and element cost 11-21 %, a finiteness test in the first-element path 4 % (profiles/r04n_*,
    // r04o_*): they enter the block sums (K stays finite - finite_shift() - so S1 becomes +inf / -inf / NaN by their signs) and
    // acc_fold() moves a non-finite S1 into M2 instead of folding the block. The finite
    // elements of such a block (at most 63 per lane) are dropped: the mean and the unweighted std are NumPy's regardless; the weighted
    // std's "inf or 0" (mom_finish) then rests on the finite elements of all other blocks.
    if constexpr (HM_PAIR_EXEC != 0) {
        // EXEC-masked form: the lanes whose element NumPy's nan-functions skip sit out the accumulation (a real branch - the empty volatile asm
        // keeps the compiler from turning it back into selects, which cost 4-6 of the 19 VALU instructions of a state and element; the branch
        // itself is scalar-unit work). Same arithmetic on the participating lanes: the same bits.
        if (use) {
            asm volatile("" ::: "memory");
            if constexpr (!LEAN) {
                if (!a.haveK) {                       // (elements of weight 0 - std = inf - have added nothing: K is re-taken until one counts)
                    asm volatile("" ::: "memory");
                    a.K = finite_shift(v);            // (weighted_first() here costs the std kernel 12 bytes of scratch and 11 %: 2 410 -> 2 670 us)
                    a.haveK = WEIGHTED ? (w != 0.0) : true;
                }
            }
            const double d = v - a.K;
            if constexpr (WEIGHTED) {
                const double t = w * d;
                a.S0 += w; a.S1 += t; a.S2 = fma(t, d, a.S2);
            } else {
                a.S0 += 1.0; a.S1 += d; a.S2 = fma(d, d, a.S2);
            }
        }
        return;
    }
    if constexpr (!LEAN) {
        a.K = (!a.haveK && use) ? finite_shift(v) : a.K;
        a.haveK = a.haveK || (use && (!WEIGHTED || w != 0.0));
    }
    const double d = use ? v - a.K : 0.0;
    if constexpr (WEIGHTED) {
        const double we = use ? w : 0.0;
        const double t = we * d;
        a.S0 += we; a.S1 += t; a.S2 = fma(t, d, a.S2);
    } else {
        a.S0 += use ? 1.0 : 0.0; a.S1 += d; a.S2 = fma(d, d, a.S2);
    }
}

// Chan / Golub / LeVeque pairwise combination; an empty side (W == 0) leaves the other's moments untouched
__device__ __forceinline__ Mom mom_merge(const Mom& a, const Mom& b) {
    Mom r;
    r.Wall = a.Wall + b.Wall; r.ss = a.ss + b.ss; r.cs = a.cs + b.cs;
    if (b.W == 0.0) { r.W = a.W; r.mean = a.mean; r.M2 = a.M2 + b.M2; return r; }      // (an empty side's M2 is 0 - or the sum of its infinite terms)
    if (a.W == 0.0) { r.W = b.W; r.mean = b.mean; r.M2 = b.M2 + a.M2; return r; }
    const double W = a.W + b.W;
    const double d = b.mean - a.mean;
    const double f = b.W / W;
    r.W = W;
    r.mean = a.mean + d * f;
    r.M2 = (a.M2 + b.M2) + (d * d) * (a.W * f);
    return r;
}

__device__ __forceinline__ Mom mom_shfl_down(const Mom& m, int off) {
    Mom r;
    r.Wall = __shfl_down(m.Wall, off, 64); r.W = __shfl_down(m.W, off, 64); r.mean = __shfl_down(m.mean, off, 64);
    r.M2 = __shfl_down(m.M2, off, 64); r.ss = __shfl_down(m.ss, off, 64); r.cs = __shfl_down(m.cs, off, 64);
    return r;
}
__device__ __forceinline__ void mom_store(double* p, const Mom& m) { p[0] = m.Wall; p[1] = m.W; p[2] = m.mean; p[3] = m.M2; p[4] = m.ss; p[5] = m.cs; }
__device__ __forceinline__ Mom mom_load(const double* p) { return Mom{p[0], p[1], p[2], p[3], p[4], p[5]}; }

// workgroup-level combination of one state per thread, where thread t's state belongs to channel `ct`:
// per channel a shuffle tree inside each wave (lanes of other channels contribute the empty state), then the four waves in order.
// Result for channel c is written to partial[(block * HM_MAX_CHANNELS + c) * nq + q] by thread c (q = quantity index).
template <int NQ>
__device__ __forceinline__ void block_merge_store(const Mom (&mine)[NQ], int ct, double* partial) {
    __shared__ double red[4][HM_MAX_CHANNELS][NQ][kMomVals];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < HM_MAX_CHANNELS; ++c) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            Mom m = c == ct ? mine[q] : mom_zero();
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = mom_merge(m, mom_shfl_down(m, off));
            if (lane == 0) mom_store(red[wave][c][q], m);
        }
    }
    __syncthreads();
    if (threadIdx.x < HM_MAX_CHANNELS * NQ) {
        const int c = threadIdx.x / NQ, q = threadIdx.x % NQ;
        Mom m = mom_load(red[0][c][q]);
        for (int w = 1; w < 4; ++w) m = mom_merge(m, mom_load(red[w][c][q]));
        mom_store(partial + ((static_cast<int64_t>(blockIdx.x) * HM_MAX_CHANNELS + c) * NQ + q) * kMomVals, m);
    }
}

// grid-level combination (one workgroup): thread t folds blocks t, t + 256, ... in order, then a fixed LDS tree over the 256 threads
template <int NQ>
__device__ __forceinline__ Mom grid_merge(const double* __restrict__ partial, int nblocks, int c, int q) {
    __shared__ double tree[256][kMomVals];
    Mom m = mom_zero();
    for (int b = threadIdx.x; b < nblocks; b += 256)
        m = mom_merge(m, mom_load(partial + ((static_cast<int64_t>(b) * HM_MAX_CHANNELS + c) * NQ + q) * kMomVals));
    __syncthreads();                                        // (the previous (c, q) round is done with `tree`)
    mom_store(tree[threadIdx.x], m);
    __syncthreads();
    for (int span = 128; span > 0; span >>= 1) {
        if (static_cast<int>(threadIdx.x) < span) {
            const Mom r = mom_merge(mom_load(tree[threadIdx.x]), mom_load(tree[threadIdx.x + span]));
            mom_store(tree[threadIdx.x], r);
        }
        __syncthreads();
    }
    return mom_load(tree[0]);
}

// mean / std / error of modules/measurand.py:339-349 from the combined state:
//   mean = nansum(v w) / nansum(w) = W mean_W / Wall;  std = sqrt(nansum(w (v - mean)^2) / nansum(w));  error = nanmean(std)
__device__ __forceinline__ void mom_finish(const Mom& m, bool weighted, double& mean, double& sd, double& err) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!is_finite(m.M2)) {
        // a term v * w was infinite; m.M2 is the sum of those terms (+inf, -inf, NaN for both signs). What NumPy then computes:
        //   nanmean / nansum(v w) / nansum(w): the infinite sum over the count or the weights;  nanstd: (v - mean) is inf - inf = NaN for the
        //   infinite element and the reduction there is a plain sum -> NaN;  weighted: nansum(w (v - mean)^2) SKIPS the NaN terms - with
        //   mean = +-inf every finite element with w > 0 contributes inf (sum inf, or 0 when there is none), with mean = NaN every term is
        //   skipped (sum 0) - over nansum(w).
        mean = m.M2 / m.Wall;
        if (!weighted) sd = nan;
        else sd = sqrt(((mean == mean && m.W > 0.0) ? __longlong_as_double(0x7ff0000000000000ll) : 0.0) / m.Wall);
        err = weighted ? m.ss / m.cs : nan;
        return;
    }
    // sum w (v - mean)^2 has the sign of the weights: rounding in S2 - S1^2 / S0 may leave -1e-13 on the other side of 0 where the data have no
    // spread. Stds that are all negative give w = 1 / std < 0 throughout: M2 and Wall are both negative and the reference's std is the
    // ordinary positive one (measurand.py:342-346) - an unconditional max(M2, 0) made it 0.
    const double M2 = m.W < 0.0 ? fmin(m.M2, 0.0) : fmax(m.M2, 0.0);
    if (m.Wall == m.W) { mean = m.W == 0.0 ? nan : m.mean; sd = sqrt(M2 / m.Wall); }
    else {                                                  // some weights belong to NaN values: the reference's denominators still count them
        mean = (m.W * m.mean) / m.Wall;
        const double d = m.mean - mean;
        sd = sqrt((M2 + m.W * (d * d)) / m.Wall);
    }
    err = weighted ? m.ss / m.cs : nan;
}

// 8-byte load at (wave-uniform base) + (32-bit byte offset in a VGPR): one 64-bit add per load, no per-lane index arithmetic
template <bool NT>
__device__ __forceinline__ double ld_f64_sv(const double* sbase, uint32_t byte_off) {
    typedef const __attribute__((address_space(1))) double* gdp;
    typedef const __attribute__((address_space(1))) char* gcp;
    gdp p = (gdp)((gcp)sbase + byte_off);
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// 1 / s as the IEEE division gives it, without the division's operand scaling and fix-up instructions: the estimate, two Newton
// steps and Markstein's correction - instruction for instruction what hipcc emits for 1.0 / s minus v_div_scale_f64 (x 2) and
// v_div_fixup_f64, which are the identity for 2^-500 <= |s| <= 2^500 (hm_merge.hip: div_inrange). `special` reports a lane outside
// that range (zero, denormal, huge, infinite; a NaN needs no help); the caller then divides properly for the whole wave.
__device__ __forceinline__ double recip_inrange(double s, bool& special) {
    const double as = fabs(s);
    special = as < 0x1p-500 || as > 0x1p500;
    double r = __builtin_amdgcn_rcp(s);
    double e = fma(-s, r, 1.0);
    r = fma(r, e, r);
    e = fma(-s, r, 1.0);
    r = fma(r, e, r);
    const double q = 1.0 * r;
    const double res = fma(-s, q, 1.0);
    return fma(res, r, q);
}

}  // namespace hm
