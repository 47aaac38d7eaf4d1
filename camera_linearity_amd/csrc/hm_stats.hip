// hm_stats.hip - the mean / std statistics of the linearity path as HIP kernels (gfx950), with their _workspace_bytes:
//   hm_channel_statistics    compute_dimension_statistics(axis = all but the last)   modules/measurand.py:318-350
//   hm_pair_statistics       ExposurePair.compute_difference + compute_stats(axis=(0,1)) of one pair      modules/exposure_series.py:33-54
//   hm_pairs_statistics      the same for every pair of a stack (ExposureSeries.process_linearity)         modules/exposure_series.py:421-446
// Streaming, HBM-bound; the statistics are ONE deterministic reduction pass (per-thread Welford states combined with Chan's
// formula by wave shuffles + LDS, then one workgroup), NaNs ignored exactly as np.nansum / np.nanmean / np.nanstd do.
// The moments themselves: hm_moments.h; the pair arithmetic: hm_stats_pairs_dev.h. The row's other units: hm_pointwise.hip, hm_stats_hist.hip,
// hm_stats_axis.hip, hm_stats_dn.hip (the all-pairs statistics straight from DN frames).
#include "hm_moments.h"
#include "hm_stats_pairs.h"
#include "hm_stats_pairs_dev.h"
#include "hm_pointwise.h"

namespace hm {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// The launch uses a total thread count that is a multiple of C (grid rounded to a multiple of 12 workgroups), so a lane's
// elements all have the same channel ct = first_element % C. A wave walks over 64-element chunks (sb, sb + stride, ...: four per
// iteration), whole chunks on a select-free path with the next iteration's loads issued before the current one's arithmetic (two
// register sets, unconditional prefetch: see pair_loop), the last partial ones with their missing elements at weight 0.
#ifndef HM_STATS_UN_NOSTD
#define HM_STATS_UN_NOSTD 8
#endif
template <bool WEIGHTED>
__device__ __forceinline__ Mom stats_loop(const double* val, const double* sd, int64_t n, int64_t sb0, int64_t stride, uint32_t lane) {
    constexpr int UN = WEIGHTED ? 4 : HM_STATS_UN_NOSTD;     // 64-element chunks per iteration (one stream: more of them in flight; same fold points)
    MomAcc st = acc_zero();
    const uint32_t lo = lane * 8u;
    int it = 0;
    int64_t sb = sb0;
    auto add = [&](double v, double s, bool ok) {
        double w = 1.0;
        if constexpr (WEIGHTED) {                           // w = 1 / std, measurand.py:342
            bool special;
            w = recip_inrange(s, special);
            if (__builtin_amdgcn_ballot_w64(special) != 0) w = 1.0 / s;
        }
        acc_add(st, v, w, s, WEIGHTED, ok);
    };
    auto fold = [&]() { if ((it & (kMomBlock / UN - 1)) == kMomBlock / UN - 1 || it == 0) acc_fold<false>(st); };   // (it == 0: early_fold, see MomAcc)
    auto whole = [&](int64_t b) { return b + (UN - 1) * stride + 64 <= n; };
    auto load = [&](int64_t b, double (&vv)[UN], double (&sv)[UN]) {
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int64_t cb = b + u * stride;                                   // scalar
            vv[u] = ld_f64_sv<true>(val + cb, lo);
            sv[u] = WEIGHTED ? ld_f64_sv<true>(sd + cb, lo) : 1.0;
        }
    };
    auto process = [&](const double (&vv)[UN], const double (&sv)[UN]) {
#pragma unroll
        for (int u = 0; u < UN; ++u) add(vv[u], sv[u], true);
        fold();
    };
    const int64_t step = UN * stride;
    double va[UN], sa[UN], vb[UN], sbv[UN];
    if (whole(sb)) load(sb, va, sa);
    while (whole(sb)) {
        load(whole(sb + step) ? sb + step : sb, vb, sbv);
        process(va, sa);
        ++it; sb += step;
        if (!whole(sb)) break;
        load(whole(sb + step) ? sb + step : sb, va, sa);
        process(vb, sbv);
        ++it; sb += step;
    }
    for (; sb < n; sb += step, ++it) {                                           // the wave's last, partial chunks
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int64_t q = sb + u * stride + lane;
            const bool ok = q < n;
            const int64_t qc = ok ? q : n - 1;                                   // a valid address, weight 0
            add(val[qc], WEIGHTED ? sd[qc] : 1.0, ok);
        }
        fold();
    }
    return acc_finish<false>(st, WEIGHTED);
}

template <bool WEIGHTED>          // one kernel per case: each gets the registers (occupancy) and the code size of its own loop
__global__ __launch_bounds__(256) void k_stats(const double* __restrict__ val, const double* __restrict__ sd, int64_t n, int C,
                                               double* __restrict__ partial) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t sb0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
    const int ct = static_cast<int>((sb0 + lane) % C);
    const Mom mine[1] = {stats_loop<WEIGHTED>(val, sd, n, sb0, stride, lane)};
    block_merge_store<1>(mine, ct, partial);
}

__global__ __launch_bounds__(256) void k_stats_final(const double* __restrict__ partial, int nblocks, int C, int weighted,
                                                     double* __restrict__ out) {
    const int c = blockIdx.x;                               // one workgroup per channel (they ran one after the other in one workgroup: 19 us)
    const Mom m = grid_merge<1>(partial, nblocks, c, 0);
    if (threadIdx.x == 0) {
        double mean, sdv, err;
        mom_finish(m, weighted != 0, mean, sdv, err);
        out[c] = mean; out[C + c] = sdv; out[2 * C + c] = err;
    }
}

// ---- pair-fused linearity statistics: the difference terms, pair_process / pair_process_any and the tail's arithmetic are
// hm_stats_pairs_dev.h (shared with hm_stats_dn.hip) ----
// the wave's last, partial chunks (from iteration `it` at element sb on) of float64 frames, then the final fold
template <bool SX, bool SY, int UN = kPairUN>
__device__ __forceinline__ void pair_tail(MomAcc (&st)[2], int it, int64_t sb, const double* x, const double* sx, const double* y,
                                          const double* sy, double mult, int64_t n, int64_t stride, uint32_t lane, Mom (&mine)[2]) {
    constexpr bool STD = SX || SY;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    pair_tail_with<STD, UN>(st, it, sb, mult, n, stride, lane, mine, [=](int64_t qc, bool ok, double& xv, double& xs, double& yv, double& ys) {
        xv = ok ? x[qc] : nan;                                                   // a valid address; the element enters as NaN
        yv = y[qc];
        xs = SX ? sx[qc] : 0.0;
        ys = SY ? sy[qc] : 0.0;
        if (STD) xs = ok ? xs : nan;
    });
}

// UN = 64-element chunks per wave iteration. Without stds a lane has only two 8-byte loads per chunk in flight: the per-pair kernel then
// takes four chunks per iteration (same element order per lane, same fold points: the same bits as UN = 2)
template <bool SX, bool SY, bool NT, int UN = kPairUN>
__device__ __forceinline__ void pair_loop(const double* x, const double* sx, const double* y, const double* sy, double mult, int64_t n,
                                          int64_t sb0, int64_t stride, uint32_t lane, Mom (&mine)[2]) {
    constexpr bool STD = SX || SY;
    MomAcc st[2] = {acc_zero(), acc_zero()};                                   // absolute | relative difference
    const uint32_t lo = lane * 8u;
    int it = 0;
    int64_t sb = sb0;
    // whole chunks (every lane exists): the next iteration's loads are issued before the current one's arithmetic (two register sets,
    // the loop written out twice) - a wave that waits for its loads at the top of every iteration leaves the VALU idle for the latency
    auto whole = [&](int64_t b) { return b + (UN - 1) * stride + 64 <= n; };
    auto load = [&](int64_t b, double (&xv)[UN], double (&xs)[UN], double (&yv)[UN], double (&ys)[UN]) {
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int64_t cb = b + u * stride;                                   // scalar
            xv[u] = ld_f64_sv<NT>(x + cb, lo);
            yv[u] = ld_f64_sv<NT>(y + cb, lo);
            xs[u] = SX ? ld_f64_sv<NT>(sx + cb, lo) : 0.0;
            ys[u] = SY ? ld_f64_sv<NT>(sy + cb, lo) : 0.0;
        }
    };
    const int64_t step = UN * stride;
    double xa[UN], ya[UN], sxa[UN], sya[UN], xb[UN], yb[UN], sxb[UN], syb[UN];
    // (the prefetch is unconditional - past the last whole iteration it re-reads the current one and the values are dropped: a branch
    // around the loads would make the compiler's wait counts assume they were skipped and wait for them before the arithmetic)
    if (whole(sb)) load(sb, xa, sxa, ya, sya);
    while (whole(sb)) {
        load(whole(sb + step) ? sb + step : sb, xb, sxb, yb, syb);
        pair_process_any<STD, UN>(st, it, mult, xa, sxa, ya, sya);
        ++it; sb += step;
        if (!whole(sb)) break;
        load(whole(sb + step) ? sb + step : sb, xa, sxa, ya, sya);
        pair_process_any<STD, UN>(st, it, mult, xb, sxb, yb, syb);
        ++it; sb += step;
    }
    pair_tail<SX, SY, UN>(st, it, sb, x, sx, y, sy, mult, n, stride, lane, mine);
}

template <bool SX, bool SY>
__global__ __launch_bounds__(256) void k_pair_stats(const double* __restrict__ x, const double* __restrict__ sx,
                                                    const double* __restrict__ y, const double* __restrict__ sy, double mult,
                                                    int64_t n, int C, double* __restrict__ partial) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;       // a multiple of C (see k_stats)
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t sb0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u);
    const int ct = static_cast<int>((sb0 + lane) % C);
    Mom mine[2];
#ifndef HM_PAIR_UN_NOSTD
#define HM_PAIR_UN_NOSTD 4
#endif
    pair_loop<SX, SY, true, (SX || SY) ? kPairUN : HM_PAIR_UN_NOSTD>(x, sx, y, sy, mult, n, sb0, stride, lane, mine);
    block_merge_store<2>(mine, ct, partial);
}

__global__ __launch_bounds__(256) void k_pair_final(const double* __restrict__ partial, int nblocks, int C, int weighted,
                                                    double* __restrict__ out) {
    const int h = blockIdx.x / C, c = blockIdx.x % C;       // one workgroup per (difference kind, channel)
    const Mom m = grid_merge<2>(partial, nblocks, c, h);
    if (threadIdx.x == 0) {
        double mean, sdv, err;
        mom_finish(m, weighted != 0, mean, sdv, err);
        double* o = out + 3 * C * h;
        o[c] = mean; o[C + c] = sdv; o[2 * C + c] = err;
    }
}

// ---- all exposure pairs of a stack in one launch ------------------------------------------------
// ExposureSeries.process_linearity (modules/exposure_series.py:421-446) evaluates compute_difference + compute_stats for every
// exposure pair (i, j) of the series: N (N - 1) / 2 pairs, each reading two frames (+ stds). Pair by pair every frame is read
// N - 1 times from HBM. Here a workgroup owns a run of elements and each of its waves owns ONE pair: the waves of a workgroup
// read the same 64-element chunks of the frames their pairs need at about the same time, so a chunk comes from HBM once and
// from the CU's L1 / the XCD's L2 for the other waves; every wave keeps the Welford states of its pair (absolute and relative
// difference) and its partial goes to partial[block][pair]. Up to HM_PAIRS_MAX pairs per launch (1024-thread workgroups).
__global__ __launch_bounds__(1024) void k_pairs_stats(const PairsK a, double* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));       // = pair index, wave-uniform
    const double* x = a.val[a.pi[wave]];
    const double* y = a.val[a.pj[wave]];
    const double* sx = a.with_std ? a.sd[a.pi[wave]] : nullptr;
    const double* sy = a.with_std ? a.sd[a.pj[wave]] : nullptr;
    const double mult = a.mult[wave];
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 64;                               // a multiple of C (grid: multiple of 12)
    const int64_t sb0 = static_cast<int64_t>(blockIdx.x) * 64;
    const int ct = static_cast<int>((sb0 + lane) % a.C);
    Mom mine[2];
    // (default cache policy on the loads: the other waves of the workgroup re-read these lines)
    if (a.with_std) pair_loop<true, true, false>(x, sx, y, sy, mult, a.n, sb0, stride, lane, mine);
    else pair_loop<false, false, false>(x, sx, y, sy, mult, a.n, sb0, stride, lane, mine);
#pragma unroll
    for (int c = 0; c < HM_MAX_CHANNELS; ++c) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            Mom m = c == ct ? mine[q] : mom_zero();
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = mom_merge(m, mom_shfl_down(m, off));
            if (lane == 0)
                mom_store(partial + (((static_cast<int64_t>(blockIdx.x) * a.n_pairs + wave) * HM_MAX_CHANNELS + c) * 2 + q) * kMomVals, m);
        }
    }
}

// The same statistics with the frames staged through LDS (the launch's usual shape: N >= 3 frames, all their pairs). In k_pairs_stats
// every wave loads its own operands: 4 global loads per wave and chunk, 60 per workgroup for 14 distinct streams, and only the waves'
// rough lock-step makes the other 46 hit in L1 / L2. Here the workgroup's threads copy each stream's two 512-byte chunks of an
// iteration ONCE into LDS (16-byte items; item t of an iteration is frame t / 64, chunk (t % 64) / 32, piece t % 32 of the value image and,
// with stds, the same piece of the std image - NI = 1 or 2 items per thread) one iteration ahead of its use into one of three LDS stages, the loads in flight during the arithmetic before;
// after one barrier per iteration every wave reads its pair's operands with conflict-free ds_read_b64. HBM sees the read-once
// traffic, 1 KB per stream in flight per CU for a whole iteration, instead of 60 wave loads that mostly hit in cache.
// THR: AbstractMeasurand.apply_thresholds (modules/measurand.py:375-428) fused into the loader, which is the one place where every element of
// every frame passes exactly once per launch: a value outside [lo, hi] of its channel becomes NaN together with its std, in the LDS copy AND in
// the frame itself (a 16-byte store where something changed) - ExposureSeries.process_linearity (modules/exposure_series.py:437-441) leaves
// its image sets thresholded. One thread stages a value item AND its std item, so the decision needs no second reader. Idempotent, so
// the dropped re-read past the last whole iteration and a second launch over the same frames change nothing.
template <bool STD, int NI, bool THR>
__global__ __launch_bounds__(1024) void k_pairs_stats_lds(const PairsK a, int n_frames, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char stage_mem[];
    const uint32_t lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));       // = pair index, wave-uniform
    const int pi = a.pi[wave], pj = a.pj[wave];
    const double mult = a.mult[wave];
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 64;                               // a multiple of C (grid: multiple of 12)
    const int64_t step = kPairUN * stride;
    const int64_t sb0 = static_cast<int64_t>(blockIdx.x) * 64;
    const int ct = static_cast<int>((sb0 + lane) % a.C);
    const int n_streams = n_frames * (STD ? 2 : 1);
    const uint32_t stage_bytes = static_cast<uint32_t>(n_streams) * 1024u;
    const int n_items = n_frames * 64;                       // an item = 16 bytes (two elements) of one frame's value chunk - and of its std chunk
    const uint32_t std_off = static_cast<uint32_t>(n_frames) * 1024u;
    // this thread's items: source pointers at iteration 0; the LDS byte offset inside a stage is item * 16 (+ std_off for the std)
    const double* src[NI];
    const double* ssrc[NI];
    bool have[NI];
    double tlo[NI][2], thi[NI][2];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int item = static_cast<int>(threadIdx.x) + k * static_cast<int>(blockDim.x);
        have[k] = item < n_items;
        const int it_ = have[k] ? item : 0;
        const int frame = it_ >> 6, u = (it_ >> 5) & 1, piece = it_ & 31;
        const int64_t e0 = sb0 + u * stride + 2 * piece;
        src[k] = a.val[frame] + e0;
        ssrc[k] = STD ? a.sd[frame] + e0 : nullptr;
        if constexpr (THR) {                                  // channels of the item's two elements: constant along the loop (step % C == 0)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = static_cast<int>((e0 + j) % a.C);
                tlo[k][j] = c == 0 ? a.lo[0] : c == 1 ? a.lo[1] : c == 2 ? a.lo[2] : a.lo[3];
                thi[k][j] = c == 0 ? a.hi[0] : c == 1 ? a.hi[1] : c == 2 ? a.hi[2] : a.hi[3];
            }
        }
    }
    auto whole = [&](int64_t b) { return b + (kPairUN - 1) * stride + 64 <= a.n; };
    struct Fetched { f64x2 v[NI]; f64x2 s[STD ? NI : 1]; int64_t delta; };
    auto fetch = [&](int64_t delta, Fetched& f) {                                               // delta = element offset of the iteration from sb0
        f.delta = delta;
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            f.v[k] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(src[k] + delta));   // read once
            if constexpr (STD) f.s[k] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(ssrc[k] + delta));
        }
    };
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    auto stash = [&](int stage, const Fetched& f) {
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            f64x2 v = f.v[k], sd = STD ? f.s[k] : f64x2{0.0, 0.0};
            if constexpr (THR) {                              // the value decides for itself and for its std (measurand.py:421-426; a NaN compares false)
                const bool m0 = v.x < tlo[k][0] || v.x > thi[k][0], m1 = v.y < tlo[k][1] || v.y > thi[k][1];
                v.x = m0 ? qnan : v.x; v.y = m1 ? qnan : v.y;
                if constexpr (STD) { sd.x = m0 ? qnan : sd.x; sd.y = m1 ? qnan : sd.y; }
                if (have[k] && (m0 || m1)) {                  // the frame itself, where it changed
                    *reinterpret_cast<f64x2*>(const_cast<double*>(src[k]) + f.delta) = v;
                    if constexpr (STD) *reinterpret_cast<f64x2*>(const_cast<double*>(ssrc[k]) + f.delta) = sd;
                }
            }
            if (have[k]) {
                char* dst = stage_mem + stage * stage_bytes + (threadIdx.x + k * blockDim.x) * 16u;
                *reinterpret_cast<f64x2*>(dst) = v;
                if constexpr (STD) *reinterpret_cast<f64x2*>(dst + std_off) = sd;
            }
        }
    };
    // a wave none of whose threads has an item (15 waves, 7 frames: items = 448 = waves 0..6) skips the loader altogether - its loads,
    // threshold selects and LDS stores were issued for nothing before: 180 of the ~3 000 VALU wave-instructions of a workgroup iteration
    const bool stager = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x & ~63u)) < n_items;          // wave-uniform
    MomAcc st[2] = {acc_zero(), acc_zero()};
    const uint32_t ox = static_cast<uint32_t>(pi) * 1024u + lane * 8u, oy = static_cast<uint32_t>(pj) * 1024u + lane * 8u;
    const uint32_t osx = ox + std_off, osy = oy + std_off;
    auto compute = [&](int stage, int it) {
        const char* sm = stage_mem + stage * stage_bytes;
        double xv[kPairUN], yv[kPairUN], xs[kPairUN], ys[kPairUN];
#pragma unroll
        for (int u = 0; u < kPairUN; ++u) {
            xv[u] = *reinterpret_cast<const double*>(sm + ox + u * 512);
            yv[u] = *reinterpret_cast<const double*>(sm + oy + u * 512);
            xs[u] = STD ? *reinterpret_cast<const double*>(sm + osx + u * 512) : 0.0;
            ys[u] = STD ? *reinterpret_cast<const double*>(sm + osy + u * 512) : 0.0;
        }
        pair_process_any<STD>(st, it, mult, xv, xs, yv, ys);
    };
    // Whole iterations (sb is the same for every wave of the workgroup, so the trip count is too). Iteration k: the registers hold
    // iteration k + 1 (loaded during iteration k - 1's arithmetic) -> LDS stage (k + 1) % 3; load iteration k + 2; barrier; compute
    // iteration k from stage k % 3. Three stages: a fast wave writes stage k + 1 while a slow one may still read stage k - 1.
    // One register set and one loop body: the only loads outstanding at the wait are the ones it is for. Past the last whole
    // iteration the prefetch re-reads the current one (dropped) - no branch around a load, see pair_loop.
    int64_t sb = sb0;
    int it = 0, stage = 0;
    Fetched r;
    auto clamp = [&](int64_t b) { return (whole(b) ? b : sb) - sb0; };
    if (whole(sb) && stager) { fetch(0, r); stash(0, r); fetch(clamp(sb + step), r); }
    while (whole(sb)) {
        const int nxt = stage == 2 ? 0 : stage + 1;
        if (stager) {
            stash(nxt, r);
            fetch(clamp(sb + 2 * step), r);
        }
        __syncthreads();
        compute(stage, it);
        ++it; sb += step; stage = nxt;
    }
    Mom mine[2];
    const double* x = a.val[pi];
    const double* y = a.val[pj];
    pair_tail<STD, STD>(st, it, sb, x, STD ? a.sd[pi] : nullptr, y, STD ? a.sd[pj] : nullptr, mult, a.n, stride, lane, mine);
#pragma unroll
    for (int c = 0; c < HM_MAX_CHANNELS; ++c) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            Mom m = c == ct ? mine[q] : mom_zero();
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = mom_merge(m, mom_shfl_down(m, off));
            if (lane == 0)
                mom_store(partial + (((static_cast<int64_t>(blockIdx.x) * a.n_pairs + wave) * HM_MAX_CHANNELS + c) * 2 + q) * kMomVals, m);
        }
    }
}

// one workgroup per pair: folds the per-block partials of its pair in a fixed order
__global__ __launch_bounds__(256) void k_pairs_final(const double* __restrict__ partial, int nblocks, int n_pairs, int C, int weighted,
                                                     double* __restrict__ out) {
    __shared__ double tree[256][kMomVals];
    const int pair = blockIdx.x;
    const int h = blockIdx.y / C, c = blockIdx.y % C;       // one workgroup per (pair, difference kind, channel)
    Mom m = mom_zero();
    for (int b = threadIdx.x; b < nblocks; b += 256)
        m = mom_merge(m, mom_load(partial + (((static_cast<int64_t>(b) * n_pairs + pair) * HM_MAX_CHANNELS + c) * 2 + h) * kMomVals));
    mom_store(tree[threadIdx.x], m);
    __syncthreads();
    for (int span = 128; span > 0; span >>= 1) {
        if (static_cast<int>(threadIdx.x) < span) {
            const Mom r = mom_merge(mom_load(tree[threadIdx.x]), mom_load(tree[threadIdx.x + span]));
            mom_store(tree[threadIdx.x], r);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double mean, sdv, err;
        mom_finish(mom_load(tree[0]), weighted != 0, mean, sdv, err);
        double* o = out + static_cast<int64_t>(pair) * 6 * C + 3 * C * h;
        o[c] = mean; o[C + c] = sdv; o[2 * C + c] = err;
    }
}

// k_pairs_final for the units that write its partial layout (declared in hm_stats_pairs.h: hm_stats_dn.hip)
void launch_pairs_final(const double* partial, int nblocks, int n_pairs, int C, int weighted, double* out, hipStream_t st) {
    hipLaunchKernelGGL(k_pairs_final, dim3(n_pairs, 2 * C), dim3(256), 0, st, partial, nblocks, n_pairs, C, weighted, out);
}

}  // namespace hm

using namespace hm;

extern "C" size_t hm_channel_statistics_workspace_bytes(void) {
    return sizeof(double) * (kStatBlocks * HM_MAX_CHANNELS * kMomVals);
}

// n counts the elements of whole pixels (n % C == 0: HM_EINVAL otherwise, on both builds). The stds of a channel are expected to have one
// sign: all negative gives the reference's statistics with error = nanmean(std) < 0; with mixed signs sum(1 / std) can cancel and
// nothing is promised.
extern "C" int hm_channel_statistics(const double* val, const double* std, int64_t n, int C,
                                     double* out /*3*C: mean, std, error*/, void* workspace, void* stream) {
    if (n < 1 || C < 1 || C > HM_MAX_CHANNELS || !val || !out || !workspace || n % C != 0) return HM_EINVAL;
    if (!aligned(val, 8) || (std && !aligned(std, 8))) return HM_EALIGN;
    double* partial = static_cast<double*>(workspace);
    const int grid = stat_grid(n, 256);
    hipStream_t st = as_stream(stream);
    if (std) hipLaunchKernelGGL(k_stats<true>, dim3(grid), dim3(256), 0, st, val, std, n, C, partial);
    else hipLaunchKernelGGL(k_stats<false>, dim3(grid), dim3(256), 0, st, val, std, n, C, partial);
    hipLaunchKernelGGL(k_stats_final, dim3(C), dim3(256), 0, st, partial, grid, C, std ? 1 : 0, out);
    return launch_status();
}

extern "C" size_t hm_pair_statistics_workspace_bytes(void) {
    return sizeof(double) * (kStatBlocks * HM_MAX_CHANNELS * 2 * kMomVals);
}

extern "C" int hm_pair_statistics(const double* x, const double* sx, const double* y, const double* sy, double multiplier,
                                  int64_t n, int C, double* out /*6*C*/, void* workspace, void* stream) {
    if (n < 1 || C < 1 || C > HM_MAX_CHANNELS || !x || !y || !out || !workspace || n % C != 0) return HM_EINVAL;
    if (!aligned(x, 8) || !aligned(y, 8) || (sx && !aligned(sx, 8)) || (sy && !aligned(sy, 8))) return HM_EALIGN;
    double* partial = static_cast<double*>(workspace);
    const int grid = stat_grid(n, 256);
    hipStream_t st = as_stream(stream);
#define HM_PAIR(A, B) hipLaunchKernelGGL((k_pair_stats<A, B>), dim3(grid), dim3(256), 0, st, x, sx, y, sy, multiplier, n, C, partial)
    if (sx && sy) HM_PAIR(true, true); else if (sx) HM_PAIR(true, false); else if (sy) HM_PAIR(false, true); else HM_PAIR(false, false);
#undef HM_PAIR
    hipLaunchKernelGGL(k_pair_final, dim3(2 * C), dim3(256), 0, st, partial, grid, C, (sx || sy) ? 1 : 0, out);
    return launch_status();
}

extern "C" size_t hm_pairs_statistics_workspace_bytes(int n_pairs) {
    const int p = n_pairs < 1 ? 1 : (n_pairs > HM_PAIRS_MAX ? HM_PAIRS_MAX : n_pairs);
    return sizeof(double) * static_cast<size_t>(kStatBlocks) * static_cast<size_t>(p) * HM_MAX_CHANNELS * 2 * kMomVals;
}

extern "C" int hm_pairs_statistics(const double* const* vals, const double* const* stds, int n_frames, const int32_t* pair_i,
                                   const int32_t* pair_j, const double* multipliers, int n_pairs, int64_t n, int C,
                                   const double* lower, const double* upper,
                                   double* out /*n_pairs * 6C*/, void* workspace, void* stream) {
    const int rc = hm_rules::check_pairs(vals, stds, n_frames, pair_i, pair_j, multipliers, n_pairs, n, C, lower, upper, out, workspace);
    if (rc != HM_OK) return rc;
    const bool thr = lower != nullptr;
    PairsK k{};
    pairs_dist_fill(k, vals, stds, n_frames, n, C, lower, upper);
    ChanLimits lim{};
    for (int c = 0; c < HM_MAX_CHANNELS; ++c) { lim.lo[c] = k.lo[c]; lim.hi[c] = k.hi[c]; }
    hipStream_t st = as_stream(stream);
    double* partial = static_cast<double*>(workspace);
    const int grid = stat_grid(n, 64);
    const int n_streams = n_frames * (stds ? 2 : 1);
    bool al16 = true;
    for (int i = 0; i < n_frames; ++i) al16 = al16 && aligned(vals[i], 16) && (!stds || aligned(stds[i], 16));
    // the thresholds (in place, as apply_thresholds does) ride on the first launch's loader when that launch stages the frames through LDS:
    // every element below `fused_end` lies in an iteration that is whole for every workgroup. The rest - and everything when the first
    // launch cannot use the LDS kernel - goes through k_thresholds first.
    auto lds_ok = [&](int np) { return al16 && n_frames * 64 <= 2 * 64 * np && n_streams <= 21; };
    const int np_first = n_pairs < HM_PAIRS_MAX ? n_pairs : HM_PAIRS_MAX;
    bool fuse_thr = false;
    if (thr) {
        const int64_t stride = static_cast<int64_t>(grid) * 64;
        int64_t whole_all = 0;                                               // iterations that are whole for the LAST workgroup (hence for all)
        while ((static_cast<int64_t>(grid) - 1) * 64 + (2 * whole_all + 1) * stride + 64 <= n) ++whole_all;
        const int64_t fused_end = lds_ok(np_first) ? 2 * stride * whole_all : 0;         // a multiple of C (stride is)
        fuse_thr = fused_end > 0;
        if (fused_end < n) {
            const int64_t m = n - fused_end;
            for (int i = 0; i < n_frames; ++i) {
                double* v = const_cast<double*>(vals[i]) + fused_end;
                double* sdp = stds ? const_cast<double*>(stds[i]) + fused_end : nullptr;
                launch_thresholds(v, sdp, lim, m, C, st);
            }
        }
    }
    for (int p0 = 0; p0 < n_pairs; p0 += HM_PAIRS_MAX) {                 // HM_PAIRS_MAX pairs (waves of a workgroup) per launch
        const int np = n_pairs - p0 < HM_PAIRS_MAX ? n_pairs - p0 : HM_PAIRS_MAX;
        k.n_pairs = np;
        for (int p = 0; p < np; ++p) { k.pi[p] = pair_i[p0 + p]; k.pj[p] = pair_j[p0 + p]; k.mult[p] = multipliers[p0 + p]; }
        // frames through LDS when a workgroup's threads can copy an iteration's 64 * n_streams 16-byte items with at most two each
        const int items = n_frames * 64, threads = 64 * np;          // one item = 16 bytes of a frame's value chunk (+ the same of its std)
        if (lds_ok(np)) {                                                                   // 3 stages x n_streams KB <= 64 KB of LDS
            const size_t lds = 3u * static_cast<size_t>(n_streams) * 1024u;
            const bool t_ = fuse_thr && p0 == 0;
#define HM_PLDS(S, N, T) hipLaunchKernelGGL((k_pairs_stats_lds<S, N, T>), dim3(grid), dim3(threads), lds, st, k, n_frames, partial)
            if (stds) {
                if (items <= threads) { if (t_) HM_PLDS(true, 1, true); else HM_PLDS(true, 1, false); }
                else { if (t_) HM_PLDS(true, 2, true); else HM_PLDS(true, 2, false); }
            } else {
                if (items <= threads) { if (t_) HM_PLDS(false, 1, true); else HM_PLDS(false, 1, false); }
                else { if (t_) HM_PLDS(false, 2, true); else HM_PLDS(false, 2, false); }
            }
#undef HM_PLDS
        } else
            hipLaunchKernelGGL(k_pairs_stats, dim3(grid), dim3(64 * np), 0, st, k, partial);
        launch_pairs_final(partial, grid, np, C, k.with_std, out + static_cast<int64_t>(p0) * 6 * C, st);
    }
    return launch_status();
}
