// hm_stats_hist_dn.hip - hm_pairs_minmax_dn, hm_pairs_histogram_dn: the all-pairs linearity distributions (hm_stats_hist.hip: hm_pairs_minmax,
// hm_pairs_histogram) straight from uint8 or uint16 DN frames (gfx950). As in hm_stats_dn.hip everything a frame element contributes is a
// function of (DN & (2^bit_depth - 1), channel): k_pairs_dn_table (hm_stats_dn.hip, through hm_stats_pairs.h) writes the thresholded
// {value, std} table once per call into the caller's workspace, behind the partials; the kernels here read DNs and gather from it. The
// frames are never written.
//   k_pairs_hist_dn      k_pairs_hist's geometry: wpp waves per pair, a grid that is a multiple of 12 workgroups (a lane keeps its channel),
//                        float64 LDS histograms [pair][kind][channel][bin], no barrier inside the loop, partials summed by k_hist_final.
//                        Only the operand source differs: two 1- or 2-byte DN loads, the mask, one gather of {v} or {v, s} each. The
//                        thresholds are in the table: there is no compare. A lane loads its next element's DNs before it works on the
//                        current one, so that the DN load and the gather that depends on it are not both in front of the arithmetic.
//   k_pairs_minmax_dn    k_pairs_minmax's geometry and reduction, the same operand source, partials folded by k_pairs_minmax_final.
// TLDS: every workgroup copies the table into LDS first - behind the histograms (hm_rules::pairs_hist_dn_tab_lds: only where the histograms
// lose nothing by it), or alone (min / max). The loads are per element throughout, so every frame alignment check_pairs_dn_args accepts is
// served by the one form. The difference expressions (diff_terms) and the counting rule (hm_stats_math.h) are hm_stats_hist.hip's: for the
// same table values the same counts, and weights of the same bits.
#include "hm_stats_pairs_dev.h"
#include "hm_stats_pairs.h"
#include "hm_ops_math.h"
#include "hm_stats_math.h"
#include <mutex>

namespace hm {

// hm_stats_hist.hip's: the column sum of the workgroups' histograms, the fold of their min / max partials
__global__ void k_hist_final(const double* __restrict__ partial, int nblocks, int nb, double* __restrict__ out);
__global__ void k_pairs_minmax_final(const double* __restrict__ partial, int nblocks, int n_pairs, int C, double* __restrict__ out);

// one pair's operand source as a wave sees it: the two frames, the table (global, or the workgroup's LDS copy), the lanes' channel
template <bool STD, bool U16, class P>
struct PairsDistDnWave {
    const void* fx; const void* fy;
    P tab;
    double mult;
    uint32_t mask, uC, ct;
    __device__ __forceinline__ void init(const PairsDnK& a, int wave, uint32_t ct_, P tab_) {
        fx = a.frame[a.pi[wave]]; fy = a.frame[a.pj[wave]];
        tab = tab_; mult = a.mult[wave]; mask = a.mask; uC = static_cast<uint32_t>(a.C); ct = ct_;
    }
    // the DNs of element q of both frames (one 1- or 2-byte load each), masked
    __device__ __forceinline__ void dns(int64_t q, uint32_t& ix, uint32_t& iy) const {
        if constexpr (U16) { ix = static_cast<const uint16_t*>(fx)[q] & mask; iy = static_cast<const uint16_t*>(fy)[q] & mask; }
        else { ix = static_cast<const uint8_t*>(fx)[q] & mask; iy = static_cast<const uint8_t*>(fy)[q] & mask; }
    }
    // the difference terms of an element from its two table entries (k_pairs_hist: PairsDistWave::element after its thresholds)
    __device__ __forceinline__ void element(uint32_t ix, uint32_t iy, double& av, double& as, double& rv, double& rs) const {
        double xv, xs, yv, ys;
        dn_entry<STD>(tab, ix * uC + ct, xv, xs);
        dn_entry<STD>(tab, iy * uC + ct, yv, ys);
        as = 0.0; rs = 0.0;
        diff_terms(xv, yv, xs, ys, mult, STD, av, rv, as, rs);
    }
};

// the workgroup's copy of the table at `dst` in LDS, in 16-byte pieces: the table's size is a multiple of 2 KiB, both copies 16-byte aligned
__device__ __forceinline__ void dn_table_to_lds(const PairsDnK& a, char* dst) {
    for (uint32_t o = threadIdx.x * 16u; o < a.table_bytes; o += blockDim.x * 16u)
        *reinterpret_cast<f64x2*>(dst + o) = *reinterpret_cast<const f64x2*>(static_cast<const char*>(a.table) + o);
}

// k_pairs_hist's counting rule (pairs_hist_count of hm_stats_hist.hip, the same text): non-finite values are skipped, with stds a std of 0
// is skipped and the weight is 1 / std, the bounded bin index
template <bool STD>
__device__ __forceinline__ void pairs_hist_dn_count(double* h, const double* __restrict__ eg, int bins, double lo, double hi, double norm,
                                                    double x, double s) {
    if (!hist_finite(x)) return;
    double w = 1.0;
    if constexpr (STD) {
        if (s == 0.0) return;                                               // measurand.py:457
        w = 1.0 / s;                                                        // :460
    }
    if (!hist_in_range(x, lo, hi)) return;
    atomicAdd(&h[hist_bin_bounded(x, lo, norm, eg, bins)], w);
}

template <bool STD, bool U16, class P>
__device__ __forceinline__ void pairs_hist_dn_loop(const PairsDnK& a, int wave, uint32_t ct, P tab, int64_t q0, int64_t stride, double* h0,
                                                   double* h1, const double* __restrict__ e0, const double* __restrict__ e1, int bins) {
    PairsDistDnWave<STD, U16, P> w;
    w.init(a, wave, ct, tab);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double hi0 = e0[bins], hi1 = e1[bins];
    const double lo0 = hi0 > e0[0] ? e0[0] : qnan, lo1 = hi1 > e1[0] ? e1[0] : qnan;           // hi <= lo: nothing is in range
    const double norm0 = static_cast<double>(bins) / (hi0 - lo0), norm1 = static_cast<double>(bins) / (hi1 - lo1);
    if (q0 >= a.n) return;
    uint32_t ix, iy;
    w.dns(q0, ix, iy);
    for (int64_t q = q0; q < a.n; q += stride) {
        const int64_t qn = q + stride < a.n ? q + stride : q;                                  // (no branch around a load: the last trip re-reads its own)
        uint32_t nx, ny;
        w.dns(qn, nx, ny);
        double av, as, rv, rs;
        w.element(ix, iy, av, as, rv, rs);
        pairs_hist_dn_count<STD>(h0, e0, bins, lo0, hi0, norm0, av, as);
        pairs_hist_dn_count<STD>(h1, e1, bins, lo1, hi1, norm1, rv, rs);
        ix = nx; iy = ny;
    }
}

// LDS: [pair of the launch][kind][channel][bin] float64 (a multiple of 16 bytes), then with TLDS the table
template <bool STD, bool U16, bool TLDS>
__global__ __launch_bounds__(1024) void k_pairs_hist_dn(const PairsDnK a, int wpp, int chan_mask, const double* __restrict__ edges, int bins,
                                                        double* __restrict__ partial /*[grid][n_pairs * 2 * C * bins]*/) {
    extern __shared__ __attribute__((aligned(16))) char hist_mem[];
    double* ph = reinterpret_cast<double*>(hist_mem);
    const int nb = a.n_pairs * 2 * a.C * bins;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) ph[i] = 0.0;
    const char* lds_tab = hist_mem + static_cast<uint32_t>(nb) * 8u;
    if constexpr (TLDS) dn_table_to_lds(a, hist_mem + static_cast<uint32_t>(nb) * 8u);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int wave = wv / wpp;                                                                 // = pair index of the launch, wave-uniform
    const int64_t stride = static_cast<int64_t>(gridDim.x) * wpp * 64;                         // a multiple of C (grid: multiple of 12)
    const int64_t sb0 = (static_cast<int64_t>(blockIdx.x) * wpp + wv % wpp) * 64;
    const int ct = static_cast<int>((sb0 + lane) % a.C);
    if ((chan_mask >> ct) & 1) {                                                               // (no barrier inside)
        const int64_t row = static_cast<int64_t>(wave) * 2 * a.C + ct;                         // kind 0; kind 1 is a.C rows further
        const double* e0 = edges + row * (bins + 1);
        const double* e1 = e0 + static_cast<int64_t>(a.C) * (bins + 1);
        double* h0 = ph + row * bins;
        double* h1 = h0 + a.C * bins;
        if constexpr (TLDS) pairs_hist_dn_loop<STD, U16>(a, wave, static_cast<uint32_t>(ct), lds_tab, sb0 + lane, stride, h0, h1, e0, e1, bins);
        else pairs_hist_dn_loop<STD, U16>(a, wave, static_cast<uint32_t>(ct), static_cast<const char*>(a.table), sb0 + lane, stride, h0, h1, e0, e1, bins);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += blockDim.x) partial[static_cast<int64_t>(blockIdx.x) * nb + i] = ph[i];
}

template <bool STD, bool U16, class P>
__device__ __forceinline__ void pairs_minmax_dn_loop(const PairsDnK& a, int wave, uint32_t ct, P tab, int64_t q0, int64_t stride, double (&mn)[2],
                                                     double (&mx)[2]) {
    PairsDistDnWave<STD, U16, P> w;
    w.init(a, wave, ct, tab);
    for (int64_t q = q0; q < a.n; q += stride) {
        uint32_t ix, iy;
        w.dns(q, ix, iy);
        double v[2], s[2];
        w.element(ix, iy, v[0], s[0], v[1], s[1]);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bool use = hist_finite(v[k]) && !(STD && s[k] == 0.0);
            mn[k] = use ? fmin(mn[k], v[k]) : mn[k];
            mx[k] = use ? fmax(mx[k], v[k]) : mx[k];
        }
    }
}

// k_pairs_minmax on DN frames: one wave per pair; LDS holds nothing but (TLDS) the table
template <bool STD, bool U16, bool TLDS>
__global__ __launch_bounds__(1024) void k_pairs_minmax_dn(const PairsDnK a, double* __restrict__ partial /*[grid][n_pairs][2][HM_MAX_CHANNELS][2]*/) {
    extern __shared__ __attribute__((aligned(16))) char tab_mem[];
    if constexpr (TLDS) {
        dn_table_to_lds(a, tab_mem);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 64;
    const int64_t sb0 = static_cast<int64_t>(blockIdx.x) * 64;
    const int ct = static_cast<int>((sb0 + lane) % a.C);
    double mn[2] = {1.0 / 0.0, 1.0 / 0.0}, mx[2] = {-1.0 / 0.0, -1.0 / 0.0};
    if constexpr (TLDS) pairs_minmax_dn_loop<STD, U16>(a, wave, static_cast<uint32_t>(ct), static_cast<const char*>(tab_mem), sb0 + lane, stride, mn, mx);
    else pairs_minmax_dn_loop<STD, U16>(a, wave, static_cast<uint32_t>(ct), static_cast<const char*>(a.table), sb0 + lane, stride, mn, mx);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int c = 0; c < HM_MAX_CHANNELS; ++c) {
            double lo = c == ct ? mn[k] : 1.0 / 0.0, hi = c == ct ? mx[k] : -1.0 / 0.0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { lo = fmin(lo, __shfl_down(lo, off, 64)); hi = fmax(hi, __shfl_down(hi, off, 64)); }
            if (lane == 0) {
                double* p = partial + (((static_cast<int64_t>(blockIdx.x) * a.n_pairs + wave) * 2 + k) * HM_MAX_CHANNELS + c) * 2;
                p[0] = lo; p[1] = hi;
            }
        }
    }
}

// More dynamic LDS than a kernel gets by default (histograms above 64 KiB, or the table beside them): every instantiation is given the
// CU's, once per process, on the first call of either entry (host-side, no stream work: capturable).
#define HM_HDN_EACH(X) X(false, false, false) X(false, false, true) X(false, true, false) X(false, true, true) X(true, false, false) \
                       X(true, false, true) X(true, true, false) X(true, true, true)
static int pairs_hist_dn_lds_limit() {
    static std::once_flag once;
    static int status = HM_OK;
    std::call_once(once, [] {
#define HM_HDN_FN(S, U, T) reinterpret_cast<const void*>(&k_pairs_hist_dn<S, U, T>), reinterpret_cast<const void*>(&k_pairs_minmax_dn<S, U, T>),
        const void* fns[] = {HM_HDN_EACH(HM_HDN_FN)};
#undef HM_HDN_FN
        for (const void* fn : fns)
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds) != hipSuccess) { (void)hipGetLastError(); status = HM_ELAUNCH; }
    });
    return status;
}

static void set_pairs(PairsDnK& k, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int p0, int np) {
    k.n_pairs = np;
    for (int p = 0; p < np; ++p) { k.pi[p] = pair_i[p0 + p]; k.pj[p] = pair_j[p0 + p]; k.mult[p] = multipliers[p0 + p]; }
}

}  // namespace hm

using namespace hm;

// hm_pairs_histogram's workspace (the histogram partials of the largest launch or the min / max partials), then (16-byte aligned) the
// largest table of the depth
extern "C" size_t hm_pairs_histogram_dn_workspace_bytes(int n_pairs, int bins, int C, int bit_depth) {
    const int b = bit_depth < 8 ? 8 : (bit_depth > 16 ? 16 : bit_depth);
    const int c = C < 1 ? 1 : (C > HM_MAX_CHANNELS ? HM_MAX_CHANNELS : C);
    return hm_pairs_histogram_workspace_bytes(n_pairs, bins, C) + 16 + static_cast<size_t>(hm_rules::pairs_dn_table_bytes(b, c, true));
}

extern "C" int hm_pairs_minmax_dn(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff,
                                  const double* std_table, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                                  int64_t n, int C, const double* lower, const double* upper, int variant, double* out, void* workspace,
                                  void* stream) {
    using namespace hm_rules;
    const int rc = check_pairs_minmax_dn(frames, n_frames, bit_depth, icrf, icrf_diff, std_table, pair_i, pair_j, multipliers, n_pairs, n, C,
                                         lower, upper, variant, out, workspace);
    if (rc != HM_OK) return rc;
    const bool with_std = std_table != nullptr, u16 = bit_depth > 8;
    const bool tab_lds = pairs_minmax_dn_tab_lds(bit_depth, C, with_std, variant);
    if (tab_lds)
        if (const int lrc = pairs_hist_dn_lds_limit(); lrc != HM_OK) return lrc;
    hipStream_t st = as_stream(stream);
    double* partial = static_cast<double*>(workspace);
    char* table = pairs_dn_table_at(workspace, static_cast<size_t>(pairs_minmax_partial_bytes()));      // (whatever bins the workspace was sized for)
    launch_pairs_dn_table(icrf, icrf_diff, std_table, lower, upper, bit_depth, C, table, st);
    PairsDnK k{};
    pairs_dn_fill(k, frames, n_frames, bit_depth, with_std, n, C, table);
    const size_t lds = tab_lds ? k.table_bytes : 0u;
    for (int p0 = 0; p0 < n_pairs; p0 += HM_PAIRS_MAX) {
        const int np = n_pairs - p0 < HM_PAIRS_MAX ? n_pairs - p0 : HM_PAIRS_MAX;
        set_pairs(k, pair_i, pair_j, multipliers, p0, np);
        int per_cu = kPairsDistWavesPerCU / np < kPairsDistMaxPerCU ? kPairsDistWavesPerCU / np : kPairsDistMaxPerCU;
        if (tab_lds && static_cast<int>(kPairsDnLdsBytes / static_cast<int64_t>(lds)) < per_cu) per_cu = static_cast<int>(kPairsDnLdsBytes / static_cast<int64_t>(lds));
        const int grid = pairs_dist_grid(n, per_cu, 64);
        const int key = (with_std ? 4 : 0) | (u16 ? 2 : 0) | (tab_lds ? 1 : 0);
#define HM_HDN_CASE(S, U, T) \
        case ((S) ? 4 : 0) | ((U) ? 2 : 0) | ((T) ? 1 : 0): \
            hipLaunchKernelGGL((k_pairs_minmax_dn<S, U, T>), dim3(grid), dim3(64 * np), lds, st, k, partial); break;
        switch (key) { HM_HDN_EACH(HM_HDN_CASE) }
#undef HM_HDN_CASE
        hipLaunchKernelGGL(k_pairs_minmax_final, dim3((np * 2 * C + 255) / 256), dim3(256), 0, st, partial, grid, np, C,
                           out + static_cast<int64_t>(p0) * 2 * C * 2);
    }
    return launch_status();
}

extern "C" int hm_pairs_histogram_dn(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff,
                                     const double* std_table, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers,
                                     int n_pairs, int64_t n, int C, int channel_mask, const double* lower, const double* upper,
                                     const double* edges, int bins, int variant, double* out, void* workspace, void* stream) {
    using namespace hm_rules;
    const int rc = check_pairs_histogram_dn(frames, n_frames, bit_depth, icrf, icrf_diff, std_table, pair_i, pair_j, multipliers, n_pairs, n, C,
                                            channel_mask, lower, upper, edges, bins, variant, out, workspace);
    if (rc != HM_OK) return rc;
    const bool with_std = std_table != nullptr, u16 = bit_depth > 8;
    if (const int lrc = pairs_hist_dn_lds_limit(); lrc != HM_OK) return lrc;
    hipStream_t st = as_stream(stream);
    double* partial = static_cast<double*>(workspace);
    char* table = pairs_dn_table_at(workspace, hm_pairs_histogram_workspace_bytes(n_pairs, bins, C));
    launch_pairs_dn_table(icrf, icrf_diff, std_table, lower, upper, bit_depth, C, table, st);
    PairsDnK k{};
    pairs_dn_fill(k, frames, n_frames, bit_depth, with_std, n, C, table);
    const PairsHistDnPlan plan = pairs_hist_dn_plan(n_pairs, bins, C, bit_depth, with_std, variant);
    const int64_t pair_bins = int64_t{2} * C * bins;
    for (int p0 = 0; p0 < n_pairs; p0 += plan.per) {
        const int np = n_pairs - p0 < plan.per ? n_pairs - p0 : plan.per;
        set_pairs(k, pair_i, pair_j, multipliers, p0, np);
        const bool tab_lds = pairs_hist_dn_tab_lds(plan, np, bins, C, bit_depth, with_std, variant);
        const int nb = static_cast<int>(np * pair_bins);
        const size_t lds = static_cast<size_t>(nb) * sizeof(double) + (tab_lds ? k.table_bytes : 0u);
        const int wpp = pairs_hist_wpp(np);
        const int grid = pairs_dist_grid(n, pairs_hist_per_cu(np, static_cast<int64_t>(lds)), 64 * wpp);
        const double* eg = edges + static_cast<int64_t>(p0) * 2 * C * (bins + 1);
        const int key = (with_std ? 4 : 0) | (u16 ? 2 : 0) | (tab_lds ? 1 : 0);
#define HM_HDN_CASE(S, U, T) \
        case ((S) ? 4 : 0) | ((U) ? 2 : 0) | ((T) ? 1 : 0): \
            hipLaunchKernelGGL((k_pairs_hist_dn<S, U, T>), dim3(grid), dim3(64 * np * wpp), lds, st, k, wpp, channel_mask, eg, bins, partial); break;
        switch (key) { HM_HDN_EACH(HM_HDN_CASE) }
#undef HM_HDN_CASE
        hipLaunchKernelGGL(k_hist_final, dim3((nb + 255) / 256), dim3(256), 0, st, partial, grid, nb, out + p0 * pair_bins);
    }
    return launch_status();
}

extern "C" int hm_pairs_histogram_dn_describe(int64_t n, int n_frames, int n_pairs, int C, int with_std, int bit_depth, int bins, int variant,
                                              char* buf, int buf_len) {
    if (!buf || buf_len < 1) return HM_EINVAL;
    buf[0] = '\0';
    const int rc = hm_rules::check_pairs_hist_dn_counts(n_frames, n_pairs, n, C, with_std != 0, bit_depth, bins, variant);
    if (rc != HM_OK) return rc;
    hm_rules::pairs_hist_dn_describe(n_pairs, C, with_std != 0, bit_depth, bins, variant, buf, buf_len);
    return HM_OK;
}
