// hm_stats_dn.hip - hm_pairs_statistics_dn: the all-pairs linearity statistics (hm_stats.hip: hm_pairs_statistics) straight from uint8 or
// uint16 DN frames (gfx950). Everything the pair arithmetic needs of a frame element is a function of (DN & (2^bit_depth - 1), channel):
//   v = ICRF[idx, c], s = ICRF_diff[idx, c] * STD_table[idx, c] (modules/measurand.py:512 after calculate_numerical_STD), both NaN where
//   apply_thresholds (measurand.py:375-428) excludes v.
// k_pairs_dn_table writes that thresholded table once per call into the caller's workspace (8 or 16 bytes per (idx, c)); the statistics
// kernels read DNs and gather from it. The frames are never written. The arithmetic of a wave, its element order and its fold points are
// hm_stats_pairs_dev.h, the partial layout and k_pairs_final are hm_stats.hip's: for the same operand values the same bits as
// hm_pairs_statistics on frames materialised by hm_linearize_*.
//   k_pairs_stats_dn_lds    k_pairs_stats_lds' geometry, three LDS stages and one barrier per iteration; the loader reads an item's two DNs
//                           (one 2-byte load for uint8, one 4-byte load for uint16), gathers their entries - from a copy of the table in LDS
//                           beside the stages where hm_rules::pairs_dn_table_fits_lds, else from the workspace table - and stores float64
//                           into the stage. The DN load runs three iterations ahead of its use and the gather two: both are in flight
//                           during an iteration's arithmetic, whichever memory the table is in.
//   k_pairs_stats_dn_wave   every wave loads and gathers for itself (k_pairs_stats' role): frames that are not item-aligned, more than 21
//                           streams, too few threads for the items - and, inside the staged kernel, the same loop for the element tail.
#include "hm_stats_pairs_dev.h"
#include "hm_stats_pairs.h"
#include "hm_stats_math.h"
#include <mutex>

namespace hm {

struct DnLimits { double lo[HM_MAX_CHANNELS], hi[HM_MAX_CHANNELS]; };

template <bool STD>
__global__ __launch_bounds__(256) void k_pairs_dn_table(const double* __restrict__ icrf, const double* __restrict__ icrf_diff,
                                                        const double* __restrict__ std_table, const DnLimits lim, int entries, int C,
                                                        void* __restrict__ table) {
    const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= entries) return;
    const int c = i % C;
    const double lo = c == 0 ? lim.lo[0] : c == 1 ? lim.lo[1] : c == 2 ? lim.lo[2] : lim.lo[3];
    const double hi = c == 0 ? lim.hi[0] : c == 1 ? lim.hi[1] : c == 2 ? lim.hi[2] : lim.hi[3];
    double v, s;
    pairs_dn_entry(icrf, icrf_diff, STD ? std_table : nullptr, i, lo, hi, v, s);
    if constexpr (STD) static_cast<f64x2*>(table)[i] = f64x2{v, s};
    else static_cast<double*>(table)[i] = v;
}

// element q of a frame through the workspace table: what the per-wave loop and the tail read
template <bool STD, bool U16>
__device__ __forceinline__ void dn_element(const PairsDnK& a, const void* frame, int64_t q, uint32_t c, double& v, double& s) {
    const uint32_t idx = U16 ? (static_cast<const uint16_t*>(frame)[q] & a.mask) : static_cast<const uint8_t*>(frame)[q];
    dn_entry<STD>(static_cast<const char*>(a.table), idx * static_cast<uint32_t>(a.C) + c, v, s);
}

// the wave's last, partial chunks; a lane past the end reads element n - 1 (with ITS channel, as a float64 frame would give it)
template <bool STD, bool U16>
__device__ __forceinline__ void dn_tail(const PairsDnK& a, MomAcc (&st)[2], int it, int64_t sb, const void* fx, const void* fy, double mult,
                                        int64_t stride, uint32_t lane, uint32_t ct, Mom (&mine)[2]) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const uint32_t c_last = static_cast<uint32_t>((a.n - 1) % a.C);
    pair_tail_with<STD, kPairUN>(st, it, sb, mult, a.n, stride, lane, mine, [&](int64_t qc, bool ok, double& xv, double& xs, double& yv, double& ys) {
        const uint32_t c = ok ? ct : c_last;
        dn_element<STD, U16>(a, fx, qc, c, xv, xs);
        dn_element<STD, U16>(a, fy, qc, c, yv, ys);
        xv = ok ? xv : nan;
        if (STD) xs = ok ? xs : nan;
    });
}

// a wave's two partials (absolute | relative difference; the lanes' channel ct) to partial[block][pair = wave][channel][kind]: the layout
// k_pairs_final folds
__device__ __forceinline__ void dn_store_partial(const Mom (&mine)[2], uint32_t ct, uint32_t lane, int wave, int n_pairs, double* __restrict__ partial) {
#pragma unroll
    for (int c = 0; c < HM_MAX_CHANNELS; ++c) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            Mom m = static_cast<uint32_t>(c) == ct ? mine[q] : mom_zero();
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = mom_merge(m, mom_shfl_down(m, off));
            if (lane == 0)
                mom_store(partial + (((static_cast<int64_t>(blockIdx.x) * n_pairs + wave) * HM_MAX_CHANNELS + c) * 2 + q) * kMomVals, m);
        }
    }
}

template <bool STD, bool U16>
__global__ __launch_bounds__(1024) void k_pairs_stats_dn_wave(const PairsDnK a, double* __restrict__ partial) {
    const uint32_t lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));       // = pair index, wave-uniform
    const void* fx = a.frame[a.pi[wave]];
    const void* fy = a.frame[a.pj[wave]];
    const double mult = a.mult[wave];
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 64;                               // a multiple of C (grid: multiple of 12)
    const int64_t step = kPairUN * stride;
    const int64_t sb0 = static_cast<int64_t>(blockIdx.x) * 64;
    const uint32_t ct = static_cast<uint32_t>((sb0 + lane) % a.C);
    MomAcc st[2] = {acc_zero(), acc_zero()};
    int64_t sb = sb0;
    int it = 0;
    for (; sb + (kPairUN - 1) * stride + 64 <= a.n; sb += step, ++it) {                        // whole chunks: every lane exists
        double xv[kPairUN], yv[kPairUN], xs[kPairUN], ys[kPairUN];
#pragma unroll
        for (int u = 0; u < kPairUN; ++u) {
            const int64_t q = sb + u * stride + lane;
            dn_element<STD, U16>(a, fx, q, ct, xv[u], xs[u]);
            dn_element<STD, U16>(a, fy, q, ct, yv[u], ys[u]);
        }
        pair_process_any<STD>(st, it, mult, xv, xs, yv, ys);
    }
    Mom mine[2];
    dn_tail<STD, U16>(a, st, it, sb, fx, fy, mult, stride, lane, ct, mine);
    dn_store_partial(mine, ct, lane, wave, a.n_pairs, partial);
}

// The staged form. Items, stages and barriers as k_pairs_stats_lds (hm_stats.hip): item t of an iteration is frame t / 64, chunk
// (t % 64) / 32, piece t % 32 - two consecutive elements, NI = 1 or 2 items per thread; a stage holds every frame's two value chunks and,
// with stds, its two std chunks behind them. TLDS: the table is copied into LDS behind the three stages first.
// Pipeline of a stager thread at iteration k: the gathered entries of iteration k + 1 (registers) -> stage (k + 1) % 3; the DNs of iteration
// k + 2 (registers) -> gathers issued; the DN load of iteration k + 3 issued; barrier; arithmetic of iteration k from stage k % 3. Past the
// last whole iteration the loads re-read the current one and are dropped (no branch around a load, see pair_loop).
template <bool STD, int NI, bool U16, bool TLDS>
__global__ __launch_bounds__(1024) void k_pairs_stats_dn_lds(const PairsDnK a, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char stage_mem[];
    const uint32_t lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));       // = pair index, wave-uniform
    const int pi = a.pi[wave], pj = a.pj[wave];
    const double mult = a.mult[wave];
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 64;                               // a multiple of C (grid: multiple of 12)
    const int64_t step = kPairUN * stride;
    const int64_t sb0 = static_cast<int64_t>(blockIdx.x) * 64;
    const uint32_t ct = static_cast<uint32_t>((sb0 + lane) % a.C);
    const int n_frames = a.n_frames;
    const uint32_t stage_bytes = static_cast<uint32_t>(n_frames) * (STD ? 2048u : 1024u);
    const int n_items = n_frames * 64;
    const uint32_t std_off = static_cast<uint32_t>(n_frames) * 1024u;
    const uint32_t tab_off = 3u * stage_bytes;
    const uint32_t uC = static_cast<uint32_t>(a.C);
    if constexpr (TLDS) {                                     // 16-byte pieces: the table's size is a multiple of 2 KiB, both copies 16-byte aligned
        for (uint32_t o = threadIdx.x * 16u; o < a.table_bytes; o += blockDim.x * 16u)
            *reinterpret_cast<f64x2*>(stage_mem + tab_off + o) = *reinterpret_cast<const f64x2*>(static_cast<const char*>(a.table) + o);
        __syncthreads();
    }
    // this thread's items: the source address at iteration 0 and the channels of the item's two elements (constant: step % C == 0)
    const char* src[NI];
    bool have[NI];
    uint32_t c0[NI], c1[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int item = static_cast<int>(threadIdx.x) + k * static_cast<int>(blockDim.x);
        have[k] = item < n_items;
        const int it_ = have[k] ? item : 0;
        const int frame = it_ >> 6, u = (it_ >> 5) & 1, piece = it_ & 31;
        const int64_t e0 = sb0 + u * stride + 2 * piece;
        src[k] = static_cast<const char*>(a.frame[frame]) + e0 * (U16 ? 2 : 1);
        c0[k] = static_cast<uint32_t>(e0 % a.C);
        c1[k] = c0[k] + 1u == uC ? 0u : c0[k] + 1u;
    }
    auto whole = [&](int64_t b) { return b + (kPairUN - 1) * stride + 64 <= a.n; };
    struct Raw { uint32_t r[NI]; };
    struct Gathered { f64x2 v[NI]; f64x2 s[STD ? NI : 1]; };
    auto fetch = [&](int64_t delta, Raw& f) {                                                   // delta = element offset of the iteration from sb0
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            if constexpr (U16) f.r[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(src[k] + delta * 2));   // read once
            else f.r[k] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(src[k] + delta));
        }
    };
    auto gather = [&](const Raw& f, Gathered& g) {
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            const uint32_t i0 = (U16 ? (f.r[k] & 0xffffu) : (f.r[k] & 0xffu)) & a.mask;
            const uint32_t i1 = (U16 ? (f.r[k] >> 16) : (f.r[k] >> 8)) & a.mask;
            const uint32_t at0 = i0 * uC + c0[k], at1 = i1 * uC + c1[k];
            double v0, s0, v1, s1;
            if constexpr (TLDS) {
                dn_entry<STD>(stage_mem + tab_off, at0, v0, s0);
                dn_entry<STD>(stage_mem + tab_off, at1, v1, s1);
            } else {
                dn_entry<STD>(static_cast<const char*>(a.table), at0, v0, s0);
                dn_entry<STD>(static_cast<const char*>(a.table), at1, v1, s1);
            }
            g.v[k] = f64x2{v0, v1};
            if constexpr (STD) g.s[k] = f64x2{s0, s1};
        }
    };
    auto stash = [&](int stage, const Gathered& g) {
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            if (have[k]) {
                char* dst = stage_mem + stage * stage_bytes + (threadIdx.x + k * blockDim.x) * 16u;
                *reinterpret_cast<f64x2*>(dst) = g.v[k];
                if constexpr (STD) *reinterpret_cast<f64x2*>(dst + std_off) = g.s[k];
            }
        }
    };
    // a wave none of whose threads has an item skips the loader altogether (wave-uniform)
    const bool stager = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x & ~63u)) < n_items;
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
    // Whole iterations (sb is the same for every wave of the workgroup, so the trip count is too). Three stages: a fast wave writes stage
    // k + 1 while a slow one may still read stage k - 1 (the barrier of iteration k - 1 lies between that read and the next write of it).
    int64_t sb = sb0;
    int it = 0, stage = 0;
    Raw r{};
    Gathered g{};
    auto clamp = [&](int64_t b) { return (whole(b) ? b : sb) - sb0; };
    if (whole(sb) && stager) {
        fetch(0, r); gather(r, g); stash(0, g);
        fetch(clamp(sb + step), r); gather(r, g);
        fetch(clamp(sb + 2 * step), r);
    }
    while (whole(sb)) {
        const int nxt = stage == 2 ? 0 : stage + 1;
        if (stager) {
            stash(nxt, g);
            gather(r, g);
            fetch(clamp(sb + 3 * step), r);
        }
        __syncthreads();
        compute(stage, it);
        ++it; sb += step; stage = nxt;
    }
    Mom mine[2];
    dn_tail<STD, U16>(a, st, it, sb, a.frame[pi], a.frame[pj], mult, stride, lane, ct, mine);
    dn_store_partial(mine, ct, lane, wave, a.n_pairs, partial);
}

// More dynamic LDS than a kernel gets by default: the tab=lds instantiations are given the CU's, once per process, on the first call
// that needs one (host-side, no stream work: capturable).
#define HM_DN_EACH(X) X(false, 1, false) X(false, 1, true) X(false, 2, false) X(false, 2, true) X(true, 1, false) X(true, 1, true) \
                      X(true, 2, false) X(true, 2, true)
static int pairs_dn_lds_limit() {
    static std::once_flag once;
    static int status = HM_OK;
    std::call_once(once, [] {
#define HM_DN_FN(S, N, U) reinterpret_cast<const void*>(&k_pairs_stats_dn_lds<S, N, U, true>),
        const void* fns[] = {HM_DN_EACH(HM_DN_FN)};
#undef HM_DN_FN
        for (const void* fn : fns)
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds) != hipSuccess) { (void)hipGetLastError(); status = HM_ELAUNCH; }
    });
    return status;
}

void launch_pairs_dn_table(const double* icrf, const double* icrf_diff, const double* std_table, const double* lower, const double* upper,
                           int bit_depth, int C, void* table, hipStream_t st) {
    DnLimits lim{};
    for (int c = 0; c < HM_MAX_CHANNELS; ++c) {
        lim.lo[c] = (lower && c < C) ? lower[c] : -__builtin_huge_val();
        lim.hi[c] = (upper && c < C) ? upper[c] : __builtin_huge_val();
    }
    const int entries = (1 << bit_depth) * C;
    if (std_table) hipLaunchKernelGGL(k_pairs_dn_table<true>, dim3((entries + 255) / 256), dim3(256), 0, st, icrf, icrf_diff, std_table, lim, entries, C, table);
    else hipLaunchKernelGGL(k_pairs_dn_table<false>, dim3((entries + 255) / 256), dim3(256), 0, st, icrf, icrf_diff, std_table, lim, entries, C, table);
}

}  // namespace hm

using namespace hm;

// the partials of hm_pairs_statistics, then (16-byte aligned) the largest table of the depth
extern "C" size_t hm_pairs_statistics_dn_workspace_bytes(int n_pairs, int C, int bit_depth) {
    const int b = bit_depth < 8 ? 8 : (bit_depth > 16 ? 16 : bit_depth);
    const int c = C < 1 ? 1 : (C > HM_MAX_CHANNELS ? HM_MAX_CHANNELS : C);
    return hm_pairs_statistics_workspace_bytes(n_pairs) + 16 + static_cast<size_t>(hm_rules::pairs_dn_table_bytes(b, c, true));
}

extern "C" int hm_pairs_statistics_dn(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff,
                                      const double* std_table, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers,
                                      int n_pairs, int64_t n, int C, const double* lower, const double* upper, int variant, double* out,
                                      void* workspace, void* stream) {
    using namespace hm_rules;
    const int rc = check_pairs_dn(frames, n_frames, bit_depth, icrf, icrf_diff, std_table, pair_i, pair_j, multipliers, n_pairs, n, C, lower,
                                  upper, variant, out, workspace);
    if (rc != HM_OK) return rc;
    const bool with_std = std_table != nullptr, u16 = bit_depth > 8;
    const bool item_aligned = pairs_dn_frames_item_aligned(frames, n_frames, bit_depth);
    bool any_lds = false;
    for (int p0 = 0; p0 < n_pairs; p0 += HM_PAIRS_MAX) {
        const PairsDnLaunch l = pairs_dn_launch(n_frames, n_pairs - p0 < HM_PAIRS_MAX ? n_pairs - p0 : HM_PAIRS_MAX, with_std, bit_depth, C, variant, item_aligned);
        any_lds = any_lds || (l.staged && l.tab_lds);
    }
    if (any_lds)
        if (const int lrc = pairs_dn_lds_limit(); lrc != HM_OK) return lrc;
    hipStream_t st = as_stream(stream);
    double* partial = static_cast<double*>(workspace);
    char* table = pairs_dn_table_at(workspace, hm_pairs_statistics_workspace_bytes(n_pairs));
    launch_pairs_dn_table(icrf, icrf_diff, std_table, lower, upper, bit_depth, C, table, st);
    PairsDnK k{};
    pairs_dn_fill(k, frames, n_frames, bit_depth, with_std, n, C, table);
    const int grid = stat_grid(n, 64);
    for (int p0 = 0; p0 < n_pairs; p0 += HM_PAIRS_MAX) {                 // HM_PAIRS_MAX pairs (waves of a workgroup) per launch
        const int np = n_pairs - p0 < HM_PAIRS_MAX ? n_pairs - p0 : HM_PAIRS_MAX;
        k.n_pairs = np;
        for (int p = 0; p < np; ++p) { k.pi[p] = pair_i[p0 + p]; k.pj[p] = pair_j[p0 + p]; k.mult[p] = multipliers[p0 + p]; }
        const PairsDnLaunch l = pairs_dn_launch(n_frames, np, with_std, bit_depth, C, variant, item_aligned);
        if (l.staged) {
            const size_t lds = 3u * static_cast<size_t>(n_frames) * (with_std ? 2048u : 1024u) + (l.tab_lds ? k.table_bytes : 0u);
            const int key = (with_std ? 4 : 0) | (l.ni == 2 ? 2 : 0) | (u16 ? 1 : 0);
#define HM_DN_CASE(S, N, U) \
            case ((S) ? 4 : 0) | ((N) == 2 ? 2 : 0) | ((U) ? 1 : 0): \
                if (l.tab_lds) hipLaunchKernelGGL((k_pairs_stats_dn_lds<S, N, U, true>), dim3(grid), dim3(64 * np), lds, st, k, partial); \
                else hipLaunchKernelGGL((k_pairs_stats_dn_lds<S, N, U, false>), dim3(grid), dim3(64 * np), lds, st, k, partial); \
                break;
            switch (key) { HM_DN_EACH(HM_DN_CASE) }
#undef HM_DN_CASE
        } else {
            if (with_std) { if (u16) hipLaunchKernelGGL((k_pairs_stats_dn_wave<true, true>), dim3(grid), dim3(64 * np), 0, st, k, partial);
                            else hipLaunchKernelGGL((k_pairs_stats_dn_wave<true, false>), dim3(grid), dim3(64 * np), 0, st, k, partial); }
            else { if (u16) hipLaunchKernelGGL((k_pairs_stats_dn_wave<false, true>), dim3(grid), dim3(64 * np), 0, st, k, partial);
                   else hipLaunchKernelGGL((k_pairs_stats_dn_wave<false, false>), dim3(grid), dim3(64 * np), 0, st, k, partial); }
        }
        launch_pairs_final(partial, grid, np, C, with_std ? 1 : 0, out + static_cast<int64_t>(p0) * 6 * C, st);
    }
    return launch_status();
}

extern "C" int hm_pairs_statistics_dn_describe(int64_t n, int n_frames, int n_pairs, int C, int with_std, int bit_depth, int variant,
                                               int frames_aligned, char* buf, int buf_len) {
    if (!buf || buf_len < 1) return HM_EINVAL;
    buf[0] = '\0';
    const int rc = hm_rules::check_pairs_dn_counts(n_frames, n_pairs, n, C, with_std != 0, bit_depth, variant);
    if (rc != HM_OK) return rc;
    hm_rules::pairs_dn_describe(n_frames, n_pairs, C, with_std != 0, bit_depth, variant, frames_aligned != 0, buf, buf_len);
    return HM_OK;
}
