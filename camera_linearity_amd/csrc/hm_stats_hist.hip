// hm_stats_hist.hip - histograms and min / max of the linearity path as HIP kernels (gfx950), of one image and of all exposure pairs of a stack:
//   hm_channel_histogram, hm_channel_minmax    compute_channel_histogram and its default range          modules/measurand.py:430-469
//   hm_pairs_histogram, hm_pairs_minmax        ExposurePair.process_linearity_distribution, every pair  modules/exposure_series.py:56-76
// and hm_histogram_workspace_bytes, hm_pairs_histogram_workspace_bytes.
#include "hm_stats_pairs.h"
#include "hm_ops_math.h"
#include "hm_stats_math.h"
#include <algorithm>

namespace hm {

// ---- per-channel histogram (compute_channel_histogram, modules/measurand.py:430-469) ----------------
// The counting rule of one element: hm_stats_math.h, the text the host build compiles too.
// Per-workgroup histograms in LDS (ds_add_f64), written as partials and column-summed: counts are exact,
// weighted sums reproducible up to the order of the LDS atomics inside a workgroup.
constexpr int kHistBlocks = 256;
constexpr int kHistMaxBins = 2048;        // bins * C doubles of LDS per workgroup (<= 64 KB)

__global__ __launch_bounds__(256) void k_hist(const double* __restrict__ val, const double* __restrict__ sd, int64_t n, int C,
                                              int chan_mask, const double* __restrict__ edges, int bins, double lo, double hi,
                                              double* __restrict__ partial /*[grid][C*bins]*/) {
    extern __shared__ double h[];
    const int nb = C * bins;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) h[i] = 0.0;
    __syncthreads();
    const double norm = static_cast<double>(bins) / (hi - lo);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int c = static_cast<int>(e % C);
        if (!((chan_mask >> c) & 1)) continue;
        const double x = val[e];
        if (!hist_finite(x)) continue;
        double w = 1.0;
        if (sd && !hist_weight(sd[e], w)) continue;
        if (!hist_in_range(x, lo, hi)) continue;
        atomicAdd(&h[c * bins + hist_bin(x, lo, norm, edges, bins)], w);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += blockDim.x) partial[static_cast<int64_t>(blockIdx.x) * nb + i] = h[i];
}

__global__ __launch_bounds__(256) void k_hist_final(const double* __restrict__ partial, int nblocks, int nb, double* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int b = 0; b < nblocks; ++b) s += partial[static_cast<int64_t>(b) * nb + i];
        out[i] = s;
    }
}

// per-channel min / max of the finite (and, with std, non-zero-std) values: the default range of np.histogram
__global__ __launch_bounds__(256) void k_minmax(const double* __restrict__ val, const double* __restrict__ sd, int64_t n, int C,
                                                double* __restrict__ partial /*[grid][C][2]*/) {
    __shared__ double red[4][HM_MAX_CHANNELS * 2];
    double mn[HM_MAX_CHANNELS], mx[HM_MAX_CHANNELS];
#pragma unroll
    for (int k = 0; k < HM_MAX_CHANNELS; ++k) { mn[k] = 1.0 / 0.0; mx[k] = -1.0 / 0.0; }
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int c = static_cast<int>(e % C);
        const double x = val[e];
        if (!hist_finite(x)) continue;
        if (sd && sd[e] == 0.0) continue;
#pragma unroll
        for (int k = 0; k < HM_MAX_CHANNELS; ++k) if (k == c) { mn[k] = fmin(mn[k], x); mx[k] = fmax(mx[k], x); }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < HM_MAX_CHANNELS; ++k) {
        double a = mn[k], b = mx[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { a = fmin(a, __shfl_down(a, off, 64)); b = fmax(b, __shfl_down(b, off, 64)); }
        if (lane == 0) { red[wave][2 * k] = a; red[wave][2 * k + 1] = b; }
    }
    __syncthreads();
    if (threadIdx.x < HM_MAX_CHANNELS) {
        const int k = threadIdx.x;
        partial[(blockIdx.x * HM_MAX_CHANNELS + k) * 2] = fmin(fmin(red[0][2 * k], red[1][2 * k]), fmin(red[2][2 * k], red[3][2 * k]));
        partial[(blockIdx.x * HM_MAX_CHANNELS + k) * 2 + 1] = fmax(fmax(red[0][2 * k + 1], red[1][2 * k + 1]), fmax(red[2][2 * k + 1], red[3][2 * k + 1]));
    }
}

__global__ __launch_bounds__(64) void k_minmax_final(const double* __restrict__ partial, int nblocks, int C, double* __restrict__ out /*[C][2]*/) {
    const int k = threadIdx.x;
    if (k >= C) return;
    double a = 1.0 / 0.0, b = -1.0 / 0.0;
    for (int i = 0; i < nblocks; ++i) { a = fmin(a, partial[(i * HM_MAX_CHANNELS + k) * 2]); b = fmax(b, partial[(i * HM_MAX_CHANNELS + k) * 2 + 1]); }
    out[2 * k] = a; out[2 * k + 1] = b;
}

// ---- distributions of all exposure pairs of a stack (ExposurePair.process_linearity_distribution for every pair) ----------------
// compute_difference + compute_channel_histogram of both difference images of every pair without the images: the all-pairs shape of
// k_pairs_stats - a workgroup owns a run of elements (64-element chunks sb0, sb0 + stride, ...; the grid is a multiple of 12 workgroups,
// so a lane keeps one channel), each of its waves works for ONE pair and reads its own operands, the waves of a workgroup walking the same
// chunks at about the same time: a chunk comes from HBM once and from L1 / L2 for the other waves. No LDS staging here - the LDS is
// what the histograms live in. The difference terms are k_difference's (diff_terms of hm_ops_math.h); the bin
// rule is k_hist's. Thresholds (apply_thresholds) act on the values AS READ: a value outside its channel's limits is NaN together with
// its std, the frames are not written. Without thresholds the limits are -inf / +inf, which no value is outside of.
// LDS: [pair of the launch][kind: absolute, relative][channel][bin] float64 (ds_add_f64: counts are integers below 2^53, exact).
constexpr int kPairsHistBlocks = 252;          // workgroups per CU-share of the grid: a multiple of 12 just below the 256 CUs
constexpr int kPairsHistMaxPerCU = 4;          // workgroups per CU when their LDS and wave count allow it (grid <= 4 x 252)

// one element of one pair as the kernels below see it: loaded, thresholded as read, differenced. Returns false past the end of the frames.
template <bool STD>
struct PairsDistWave {
    const double* x; const double* y; const double* sx; const double* sy;
    double mult, tlo, thi;
    __device__ __forceinline__ void init(const PairsK& a, int wave, int ct) {
        x = a.val[a.pi[wave]]; y = a.val[a.pj[wave]];
        sx = STD ? a.sd[a.pi[wave]] : nullptr; sy = STD ? a.sd[a.pj[wave]] : nullptr;
        mult = a.mult[wave];
        tlo = ct == 0 ? a.lo[0] : ct == 1 ? a.lo[1] : ct == 2 ? a.lo[2] : a.lo[3];
        thi = ct == 0 ? a.hi[0] : ct == 1 ? a.hi[1] : ct == 2 ? a.hi[2] : a.hi[3];
    }
    __device__ __forceinline__ void element(int64_t q, double& av, double& as, double& rv, double& rs) const {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double xv = x[q], yv = y[q], xs = 0.0, ys = 0.0;
        if constexpr (STD) { xs = sx[q]; ys = sy[q]; }
        const bool mx = xv < tlo || xv > thi, my = yv < tlo || yv > thi;          // measurand.py:418 (a NaN compares false: stays NaN)
        xv = mx ? nan : xv; yv = my ? nan : yv;
        if constexpr (STD) { xs = mx ? nan : xs; ys = my ? nan : ys; }
        as = 0.0; rs = 0.0;
        diff_terms(xv, yv, xs, ys, mult, STD, av, rv, as, rs);
    }
};

// k_hist's counting rule for one value into one (pair, kind, channel) histogram of `bins` LDS counters, with the index form that NO edge
// array - edges are device data nobody has checked - can take outside 0..bins-1 (hist_bin_bounded of hm_stats_math.h).
template <bool STD>
__device__ __forceinline__ void pairs_hist_count(double* h, const double* __restrict__ eg, int bins, double lo, double hi, double norm,
                                                 double x, double s) {
    if (!hist_finite(x)) return;
    double w = 1.0;
    if constexpr (STD) {                                                    // hist_weight() written out: called here, the kernel's code changes
        if (s == 0.0) return;                                               // measurand.py:457
        w = 1.0 / s;                                                        // :460
    }
    if (!hist_in_range(x, lo, hi)) return;
    atomicAdd(&h[hist_bin_bounded(x, lo, norm, eg, bins)], w);
}

template <bool STD>
__global__ __launch_bounds__(1024) void k_pairs_hist(const PairsK a, int wpp, int chan_mask, const double* __restrict__ edges, int bins,
                                                     double* __restrict__ partial /*[grid][n_pairs * 2 * C * bins]*/) {
    extern __shared__ double ph[];
    const int nb = a.n_pairs * 2 * a.C * bins;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) ph[i] = 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // wpp waves per pair (the launch's pairs rarely fill a workgroup's 16 waves: fewer pairs fit the LDS as the bins grow): wave v works for
    // pair v / wpp on the chunks blockIdx * wpp + v % wpp, + gridDim * wpp, ... - the waves of one pair add into the same LDS histograms
    const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int wave = wv / wpp;                                                                 // = pair index of the launch, wave-uniform
    const int64_t stride = static_cast<int64_t>(gridDim.x) * wpp * 64;                         // a multiple of C (grid: multiple of 12)
    const int64_t sb0 = (static_cast<int64_t>(blockIdx.x) * wpp + wv % wpp) * 64;
    const int ct = static_cast<int>((sb0 + lane) % a.C);
    if ((chan_mask >> ct) & 1) {                                                               // (no barrier inside)
        PairsDistWave<STD> w;
        w.init(a, wave, ct);
        const int64_t row = static_cast<int64_t>(wave) * 2 * a.C + ct;                         // kind 0; kind 1 is a.C rows further
        const double* e0 = edges + row * (bins + 1);
        const double* e1 = e0 + static_cast<int64_t>(a.C) * (bins + 1);
        double* h0 = ph + row * bins;
        double* h1 = h0 + a.C * bins;
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        const double hi0 = e0[bins], hi1 = e1[bins];
        const double lo0 = hi0 > e0[0] ? e0[0] : qnan, lo1 = hi1 > e1[0] ? e1[0] : qnan;       // hi <= lo (hm_channel_histogram: HM_EINVAL): nothing is in range
        const double norm0 = static_cast<double>(bins) / (hi0 - lo0), norm1 = static_cast<double>(bins) / (hi1 - lo1);
        for (int64_t q = sb0 + lane; q < a.n; q += stride) {
            double av, as, rv, rs;
            w.element(q, av, as, rv, rs);
            pairs_hist_count<STD>(h0, e0, bins, lo0, hi0, norm0, av, as);
            pairs_hist_count<STD>(h1, e1, bins, lo1, hi1, norm1, rv, rs);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += blockDim.x) partial[static_cast<int64_t>(blockIdx.x) * nb + i] = ph[i];
}

// np.histogram's default range of every (pair, kind, channel): hm_channel_minmax's rule (finite values; with stds, std != 0) on the
// difference images that are never written. Registers, then k_minmax's reduction: shuffles per channel, one partial per workgroup and pair.
template <bool STD>
__global__ __launch_bounds__(1024) void k_pairs_minmax(const PairsK a, double* __restrict__ partial /*[grid][n_pairs][2][HM_MAX_CHANNELS][2]*/) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 64;
    const int64_t sb0 = static_cast<int64_t>(blockIdx.x) * 64;
    const int ct = static_cast<int>((sb0 + lane) % a.C);
    PairsDistWave<STD> w;
    w.init(a, wave, ct);
    double mn[2] = {1.0 / 0.0, 1.0 / 0.0}, mx[2] = {-1.0 / 0.0, -1.0 / 0.0};
    for (int64_t q = sb0 + lane; q < a.n; q += stride) {
        double v[2], s[2];
        w.element(q, v[0], s[0], v[1], s[1]);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bool use = hist_finite(v[k]) && !(STD && s[k] == 0.0);
            mn[k] = use ? fmin(mn[k], v[k]) : mn[k];
            mx[k] = use ? fmax(mx[k], v[k]) : mx[k];
        }
    }
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

// one thread per (pair, kind, channel) of the launch folds the workgroups' partials in order
__global__ __launch_bounds__(256) void k_pairs_minmax_final(const double* __restrict__ partial, int nblocks, int n_pairs, int C,
                                                            double* __restrict__ out /*[n_pairs][2][C][2]*/) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pairs * 2 * C) return;
    const int c = t % C, pk = t / C;                       // pk = pair * 2 + kind
    double lo = 1.0 / 0.0, hi = -1.0 / 0.0;
    for (int b = 0; b < nblocks; ++b) {
        const double* p = partial + ((static_cast<int64_t>(b) * n_pairs * 2 + pk) * HM_MAX_CHANNELS + c) * 2;
        lo = fmin(lo, p[0]); hi = fmax(hi, p[1]);
    }
    out[2 * t] = lo; out[2 * t + 1] = hi;
}

// pairs per launch of the histogram kernel: as many (pair, 2 kinds, C channels, bins) float64 histograms as the CU's LDS holds, at most one
// per wave of a 1024-thread workgroup; always at least 1 (HM_PAIRS_HIST_MAX_BINS x HM_MAX_CHANNELS x 2 x 8 bytes = 128 KiB <= 160 KiB)
static int pairs_hist_per_launch(int bins, int C) {
    const int64_t per_pair = int64_t{2} * C * bins * static_cast<int64_t>(sizeof(double));
    const int64_t fit = kMaxLds / per_pair;
    return static_cast<int>(fit > HM_PAIRS_MAX ? HM_PAIRS_MAX : fit);
}
static_assert(int64_t{2} * HM_MAX_CHANNELS * HM_PAIRS_HIST_MAX_BINS * 8 <= kMaxLds, "one pair's histograms must fit the LDS");

// grid of the all-pairs distribution kernels: `chunk` elements (64 per wave of a pair) per workgroup and trip, a multiple of 12 workgroups
static int pairs_dist_grid(int64_t n, int per_cu, int chunk) {
    int64_t g = (n + chunk - 1) / chunk;
    g = ((g + 11) / 12) * 12;
    const int64_t cap = static_cast<int64_t>(kPairsHistBlocks) * per_cu;
    return static_cast<int>(g < cap ? g : cap);
}

}  // namespace hm

using namespace hm;

extern "C" size_t hm_histogram_workspace_bytes(int bins, int C) {
    const size_t a = sizeof(double) * static_cast<size_t>(kHistBlocks) * static_cast<size_t>(bins) * static_cast<size_t>(C);
    const size_t b = sizeof(double) * kHistBlocks * HM_MAX_CHANNELS * 2;
    return a > b ? a : b;
}

extern "C" int hm_channel_minmax(const double* val, const double* std, int64_t n, int C, double* out /*2*C*/, void* workspace,
                                 void* stream) {
    if (n < 1 || C < 1 || C > HM_MAX_CHANNELS || !val || !out || !workspace) return HM_EINVAL;
    const int grid = static_cast<int>(std::min<int64_t>(kHistBlocks, (n + 255) / 256));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_minmax, dim3(grid), dim3(256), 0, st, val, std, n, C, static_cast<double*>(workspace));
    hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(64), 0, st, static_cast<const double*>(workspace), grid, C, out);
    return launch_status();
}

extern "C" int hm_channel_histogram(const double* val, const double* std, int64_t n, int C, int channel_mask,
                                    const double* edges /*device, bins + 1*/, int bins, double lo, double hi,
                                    double* out /*C * bins*/, void* workspace, void* stream) {
    if (n < 1 || C < 1 || C > HM_MAX_CHANNELS || bins < 1 || !val || !edges || !out || !workspace || !(hi > lo)) return HM_EINVAL;
    if (bins * C > kHistMaxBins * 4) return HM_EUNSUPPORTED;
    const int nb = bins * C;
    const int lds = nb * static_cast<int>(sizeof(double));
    if (lds > 64 * 1024) return HM_EUNSUPPORTED;
    const int grid = static_cast<int>(std::min<int64_t>(kHistBlocks, (n + 255) / 256));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_hist, dim3(grid), dim3(256), lds, st, val, std, n, C, channel_mask, edges, bins, lo, hi, static_cast<double*>(workspace));
    hipLaunchKernelGGL(k_hist_final, dim3((nb + 255) / 256), dim3(256), 0, st, static_cast<const double*>(workspace), grid, nb, out);
    return launch_status();
}

// the partial histograms of the largest launch (every workgroup's LDS image: at most kMaxLds bytes each) or the min / max partials of
// a launch of HM_PAIRS_MAX pairs, whichever is larger
extern "C" size_t hm_pairs_histogram_workspace_bytes(int n_pairs, int bins, int C) {
    const size_t mm = sizeof(double) * kPairsHistBlocks * kPairsHistMaxPerCU * HM_PAIRS_MAX * 2 * HM_MAX_CHANNELS * 2;
    if (n_pairs < 1 || bins < 1 || bins > HM_PAIRS_HIST_MAX_BINS || C < 1 || C > HM_MAX_CHANNELS) return mm;
    const int ppl = pairs_hist_per_launch(bins, C);
    const size_t np = static_cast<size_t>(n_pairs < ppl ? n_pairs : ppl);
    const size_t h = sizeof(double) * kPairsHistBlocks * kPairsHistMaxPerCU * np * 2 * static_cast<size_t>(C) * static_cast<size_t>(bins);
    const size_t cap = static_cast<size_t>(kPairsHistBlocks) * kMaxLds;      // (workgroups per CU x their LDS never exceeds the CU's)
    return std::max(mm, std::min(h, cap));
}

extern "C" int hm_pairs_minmax(const double* const* vals, const double* const* stds, int n_frames, const int32_t* pair_i,
                               const int32_t* pair_j, const double* multipliers, int n_pairs, int64_t n, int C,
                               const double* lower, const double* upper, double* out, void* workspace, void* stream) {
    const int rc = hm_rules::check_pairs(vals, stds, n_frames, pair_i, pair_j, multipliers, n_pairs, n, C, lower, upper, out, workspace);
    if (rc != HM_OK) return rc;
    PairsK k{};
    pairs_dist_fill(k, vals, stds, n_frames, n, C, lower, upper);
    hipStream_t st = as_stream(stream);
    double* partial = static_cast<double*>(workspace);
    for (int p0 = 0; p0 < n_pairs; p0 += HM_PAIRS_MAX) {
        const int np = n_pairs - p0 < HM_PAIRS_MAX ? n_pairs - p0 : HM_PAIRS_MAX;
        k.n_pairs = np;
        for (int p = 0; p < np; ++p) { k.pi[p] = pair_i[p0 + p]; k.pj[p] = pair_j[p0 + p]; k.mult[p] = multipliers[p0 + p]; }
        const int per_cu = 32 / np < kPairsHistMaxPerCU ? 32 / np : kPairsHistMaxPerCU;        // 32 waves per CU
        const int grid = pairs_dist_grid(n, per_cu, 64);
        if (stds) hipLaunchKernelGGL(k_pairs_minmax<true>, dim3(grid), dim3(64 * np), 0, st, k, partial);
        else hipLaunchKernelGGL(k_pairs_minmax<false>, dim3(grid), dim3(64 * np), 0, st, k, partial);
        hipLaunchKernelGGL(k_pairs_minmax_final, dim3((np * 2 * C + 255) / 256), dim3(256), 0, st, partial, grid, np, C,
                           out + static_cast<int64_t>(p0) * 2 * C * 2);
    }
    return launch_status();
}

extern "C" int hm_pairs_histogram(const double* const* vals, const double* const* stds, int n_frames, const int32_t* pair_i,
                                  const int32_t* pair_j, const double* multipliers, int n_pairs, int64_t n, int C, int channel_mask,
                                  const double* lower, const double* upper, const double* edges, int bins, double* out, void* workspace,
                                  void* stream) {
    const int rc = hm_rules::check_pairs_histogram(vals, stds, n_frames, pair_i, pair_j, multipliers, n_pairs, n, C, channel_mask, lower, upper,
                                                   edges, bins, out, workspace);
    if (rc != HM_OK) return rc;
    PairsK k{};
    pairs_dist_fill(k, vals, stds, n_frames, n, C, lower, upper);
    hipStream_t st = as_stream(stream);
    double* partial = static_cast<double*>(workspace);
    // as many pairs per launch as the LDS holds histograms for, the launches of equal size (15 pairs at 13 per launch: 8 + 7)
    const int ppl = pairs_hist_per_launch(bins, C);
    const int launches = (n_pairs + ppl - 1) / ppl;
    const int per = (n_pairs + launches - 1) / launches;
    const int64_t pair_bins = int64_t{2} * C * bins;
    if (static_cast<size_t>(per * pair_bins) * sizeof(double) > 64 * 1024) {        // more dynamic LDS than a kernel gets by default: ask for the CU's
        const void* fn = stds ? reinterpret_cast<const void*>(&k_pairs_hist<true>) : reinterpret_cast<const void*>(&k_pairs_hist<false>);
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);      // (host-side, no stream work: capturable)
        (void)hipGetLastError();                         // a runtime that needs no such step may refuse it: the launch below decides
    }
    for (int p0 = 0; p0 < n_pairs; p0 += per) {
        const int np = n_pairs - p0 < per ? n_pairs - p0 : per;
        k.n_pairs = np;
        for (int p = 0; p < np; ++p) { k.pi[p] = pair_i[p0 + p]; k.pj[p] = pair_j[p0 + p]; k.mult[p] = multipliers[p0 + p]; }
        const int nb = static_cast<int>(np * pair_bins);
        const size_t lds = static_cast<size_t>(nb) * sizeof(double);
        int per_cu = static_cast<int>(kMaxLds / lds);                                          // workgroups a CU can hold: LDS, 32 waves
        const int wpp = HM_PAIRS_MAX / np;                                                     // waves per pair: fill the workgroup's 16 waves
        per_cu = per_cu < 32 / (np * wpp) ? per_cu : 32 / (np * wpp);
        per_cu = per_cu < kPairsHistMaxPerCU ? per_cu : kPairsHistMaxPerCU;
        const int grid = pairs_dist_grid(n, per_cu < 1 ? 1 : per_cu, 64 * wpp);
        const double* eg = edges + static_cast<int64_t>(p0) * 2 * C * (bins + 1);
        if (stds) hipLaunchKernelGGL(k_pairs_hist<true>, dim3(grid), dim3(64 * np * wpp), lds, st, k, wpp, channel_mask, eg, bins, partial);
        else hipLaunchKernelGGL(k_pairs_hist<false>, dim3(grid), dim3(64 * np * wpp), lds, st, k, wpp, channel_mask, eg, bins, partial);
        hipLaunchKernelGGL(k_hist_final, dim3((nb + 255) / 256), dim3(256), 0, st, partial, grid, nb, out + p0 * pair_bins);
    }
    return launch_status();
}
