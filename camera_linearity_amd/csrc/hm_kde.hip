// hm_kde.hip - weighted Gaussian kernel density estimates (gfx950): NumpyMeasurand.compute_kernel_density_estimate,
// modules/measurand.py:716-761 (scipy.stats.gaussian_kde(values, 'silverman', weights).evaluate(x_range), one channel at a time).
//
//   estimate[j] = sum_i p_i exp(-(u_i - v_j)^2 / 2) / (sqrt(2 pi) h),   u_i = x_i / h,  v_j = y_j / h,  p_i = w_i / sum(w)
//
// Two parts, both stream-ordered, no host sync, no allocation, no float atomics - the same inputs give the same bits on every run:
//   moments   k_kde_moments1 -> k_kde_finish -> k_kde_moments2 -> k_kde_finish: a fixed grid of kKdeMomBlocks workgroups
//             reduces count, sum w, sum w^2, sum w x, min, max and the weight flags of the counted elements into per-workgroup
//             partials, one lane-parallel pass in a fixed order writes moments[]; the second pass reads x_bar = sum w x / sum w
//             from device memory and reduces sum w (x - x_bar)^2. Bandwidth-bound and small. The host forms h from these.
//   evaluate  k_kde_eval (the hot path, FP64-exp-bound): workgroup (grid block b, chunk k) owns kKdeBlockPts grid points and a
//             contiguous span of elements. Every lane keeps kKdeG grid points (v, acc) in registers; the span is staged through
//             LDS as (u, w) tiles of kKdeTile elements and read back as same-address broadcasts. A masked element is staged as
//             u = 0, w = 0 (not multiplied by 0: NaN * 0 is NaN). exp(-a) is exactly 0 for a > 745.14, i.e. |u - v| > 38.61,
//             so a tile whose u range lies further than kKdeCut from every grid point of the workgroup is skipped: exact.
//             Partials go to workspace[chunk][m]; k_kde_sum adds the chunks in a fixed order and applies the norm.
#include "hm_common.h"
#include "hm_stats_math.h"
#include "hm_producer_rules.h"

namespace hm {

constexpr int kKdeMomBlocks = 512;             // moments: fixed grid (device-independent: same partials, same bits anywhere)
constexpr int kKdeMomThreads = 256;
constexpr int kKdeMomStride = 16;              // doubles per partial
constexpr int kKdeBlock = 256;                 // evaluate: lanes per workgroup
constexpr int kKdeG = 4;                       // grid points per lane
constexpr int kKdeBlockPts = kKdeBlock * kKdeG;
constexpr int kKdeTile = 1024;                 // elements per LDS tile (16 KiB of (u, w))
constexpr int64_t kKdeTargetChunks = 2048;     // chunks per launch (device-independent)
constexpr double kKdeCut = 38.7;               // exp(-38.7^2 / 2) = exp(-748.8) == 0.0
constexpr int kKdeSumJ = 16, kKdeSumS = 16;    // k_kde_sum: 16 grid points x 16 chunk slices per workgroup

// elements (of one channel) per chunk: a multiple of the tile, at most kKdeTargetChunks chunks
__host__ __device__ inline int64_t kde_chunk_len(int64_t n) {
    const int64_t q = n / kKdeTargetChunks + (n % kKdeTargetChunks != 0);
    const int64_t t = q / kKdeTile + (q % kKdeTile != 0);
    return (t < 1 ? 1 : t) * kKdeTile;
}
__host__ __device__ inline int64_t kde_chunks(int64_t n) {
    const int64_t len = kde_chunk_len(n);
    const int64_t k = n / len + (n % len != 0);
    return k < 1 ? 1 : k;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, kWave));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, kWave));
    return v;
}

// NV values per thread -> the workgroup's values in lds[0..NV) (fixed order: xor tree in the wave, waves in index order).
// kind[k]: 0 sum, 1 min, 2 max. Ends with a barrier; thread 0's lds values are valid everywhere.
template <int NV>
__device__ __forceinline__ void block_reduce(double (&v)[NV], const int (&kind)[NV], double* lds /* NV * waves */) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave, nw = blockDim.x / kWave;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = kind[k] == 0 ? wave_sum(v[k]) : kind[k] == 1 ? wave_min(v[k]) : wave_max(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) lds[k * 16 + wv] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double r = lds[k * 16];
            for (int q = 1; q < nw; ++q) {
                const double o = lds[k * 16 + q];
                r = kind[k] == 0 ? r + o : kind[k] == 1 ? fmin(r, o) : fmax(r, o);
            }
            lds[k * 16] = r;
        }
    }
    __syncthreads();
}

// ---- moments, pass 1: count, sum w, sum w^2, sum w x, min x, max x, #non-finite w, #w > 0, #w < 0
constexpr int kMom1 = 9;
__global__ __launch_bounds__(kKdeMomThreads) void k_kde_moments1(const double* __restrict__ val, const double* __restrict__ std,
                                                                 int64_t n, int C, int c, double* __restrict__ part) {
    __shared__ double lds[kMom1 * 16];
    double v[kMom1] = {0.0, 0.0, 0.0, 0.0, INFINITY, -INFINITY, 0.0, 0.0, 0.0};
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        double x, w;
        if (!kde_load(val, std, i * C + c, x, w)) continue;
        v[0] += 1.0;
        v[1] += w;
        v[2] += w * w;
        v[3] += w * x;
        v[4] = fmin(v[4], x);
        v[5] = fmax(v[5], x);
        v[6] += isfinite(w) ? 0.0 : 1.0;
        v[7] += w > 0.0 ? 1.0 : 0.0;
        v[8] += w < 0.0 ? 1.0 : 0.0;
    }
    const int kind[kMom1] = {0, 0, 0, 0, 1, 2, 0, 0, 0};
    block_reduce<kMom1>(v, kind, lds);
    if (threadIdx.x < kMom1) part[static_cast<int64_t>(blockIdx.x) * kKdeMomStride + threadIdx.x] = lds[threadIdx.x * 16];
}

// one wave: the kKdeMomBlocks partials of `nv` values in a fixed order -> moments[first ..] (pass 1: first = 0, min / max at 4 / 5;
// pass 2: first = 10, a sum)
__global__ __launch_bounds__(kWave) void k_kde_finish(const double* __restrict__ part, int nv, int first, double* __restrict__ moments) {
    const int lane = threadIdx.x;
    for (int k = 0; k < nv; ++k) {
        const int kind = first == 0 ? (k == 4 ? 1 : k == 5 ? 2 : 0) : 0;
        double r = kind == 1 ? INFINITY : kind == 2 ? -INFINITY : 0.0;
        for (int b = lane; b < kKdeMomBlocks; b += kWave) {
            const double o = part[static_cast<int64_t>(b) * kKdeMomStride + k];
            r = kind == 0 ? r + o : kind == 1 ? fmin(r, o) : fmax(r, o);
        }
        r = kind == 0 ? wave_sum(r) : kind == 1 ? wave_min(r) : wave_max(r);
        if (lane == 0) moments[first + k] = r;
    }
    if (first == 0 && lane == 0) moments[9] = moments[3] / moments[1];          // x_bar, read by pass 2
}

// ---- moments, pass 2: sum w (x - x_bar)^2 with x_bar = moments[9]
__global__ __launch_bounds__(kKdeMomThreads) void k_kde_moments2(const double* __restrict__ val, const double* __restrict__ std,
                                                                 int64_t n, int C, int c, const double* __restrict__ moments,
                                                                 double* __restrict__ part) {
    __shared__ double lds[16];
    const double xbar = moments[9];
    double v[1] = {0.0};
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        double x, w;
        if (!kde_load(val, std, i * C + c, x, w)) continue;
        const double d = x - xbar;
        v[0] += w * (d * d);
    }
    const int kind[1] = {0};
    block_reduce<1>(v, kind, lds);
    if (threadIdx.x == 0) part[static_cast<int64_t>(blockIdx.x) * kKdeMomStride] = lds[0];
}

// ---- evaluate
__global__ __launch_bounds__(kKdeBlock) void k_kde_eval(const double* __restrict__ val, const double* __restrict__ std, int64_t n, int C,
                                                        int c, double h, const double* __restrict__ grid, int m, int64_t chunk_len,
                                                        double* __restrict__ part) {
    __shared__ double2 tile[kKdeTile];
    __shared__ double red[2 * 16];
    const int64_t k = blockIdx.y;
    const int64_t i0 = k * chunk_len;
    const int64_t i1 = n - i0 < chunk_len ? n : i0 + chunk_len;
    const int jb = blockIdx.x * kKdeBlockPts + threadIdx.x;                  // lane's points: jb + g * kKdeBlock (coalesced stores)
    double v[kKdeG], acc[kKdeG];
    double r[2] = {INFINITY, -INFINITY};
#pragma unroll
    for (int g = 0; g < kKdeG; ++g) {
        const int j = jb + g * kKdeBlock;
        v[g] = j < m ? grid[j] / h : 0.0;
        acc[g] = 0.0;
        if (j < m) { r[0] = fmin(r[0], v[g]); r[1] = fmax(r[1], v[g]); }
    }
    const int kind[2] = {1, 2};
    block_reduce<2>(r, kind, red);
    const double vlo = red[0] - kKdeCut, vhi = red[16] + kKdeCut;        // workgroup-uniform
    const bool live = static_cast<int64_t>(blockIdx.x) * kKdeBlockPts + (threadIdx.x & ~(kWave - 1)) < m;   // wave-uniform: any point?
    for (int64_t t0 = i0; t0 < i1; t0 += kKdeTile) {
        const int cnt = i1 - t0 < kKdeTile ? static_cast<int>(i1 - t0) : kKdeTile;
        double tr[2] = {INFINITY, -INFINITY};
        __syncthreads();                                                     // the previous tile is read by every lane
        for (int q = threadIdx.x; q < cnt; q += kKdeBlock) {
            double x, w, u = 0.0;
            if (kde_load(val, std, (t0 + q) * C + c, x, w)) {
                u = x / h;
                tr[0] = fmin(tr[0], u);
                tr[1] = fmax(tr[1], u);
            } else {
                w = 0.0;
            }
            tile[q] = make_double2(u, w);
        }
        block_reduce<2>(tr, kind, red);                                      // its barriers publish the tile too
        if (red[0] > vhi || red[16] < vlo || red[0] > red[16] || !live) continue;   // every pair underflows to 0 (or nothing counted)
        for (int q = 0; q < cnt; ++q) {
            const double2 uw = tile[q];
#pragma unroll
            for (int g = 0; g < kKdeG; ++g) {
                const double d = uw.x - v[g];
                acc[g] += uw.y * exp(-(d * d) * 0.5);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < kKdeG; ++g) {
        const int j = jb + g * kKdeBlock;
        if (j < m) part[k * m + j] = acc[g];
    }
}

// out[j] = scale * sum over chunks of part[chunk][j]: slice s adds chunks s, s + 16, ... in order, then the slices in order
__global__ __launch_bounds__(kKdeSumJ * kKdeSumS) void k_kde_sum(const double* __restrict__ part, int64_t chunks, int m, double scale,
                                                                 double* __restrict__ out) {
    __shared__ double red[kKdeSumS][kKdeSumJ];
    const int jl = threadIdx.x % kKdeSumJ, s = threadIdx.x / kKdeSumJ;
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kKdeSumJ + jl;
    double a = 0.0;
    if (j < m) {
        int64_t q = s;
        for (; q + 3 * kKdeSumS < chunks; q += 4 * kKdeSumS) {
            const double p0 = part[q * m + j], p1 = part[(q + kKdeSumS) * m + j];
            const double p2 = part[(q + 2 * kKdeSumS) * m + j], p3 = part[(q + 3 * kKdeSumS) * m + j];
            a += p0; a += p1; a += p2; a += p3;
        }
        for (; q < chunks; q += kKdeSumS) a += part[q * m + j];
    }
    red[s][jl] = a;
    __syncthreads();
    if (s == 0 && j < m) {
        double t = red[0][jl];
        for (int q = 1; q < kKdeSumS; ++q) t += red[q][jl];
        out[j] = t * scale;
    }
}

}  // namespace hm

using namespace hm;

static size_t kde_eval_bytes(int64_t n, int m) { return static_cast<size_t>(kde_chunks(n)) * static_cast<size_t>(m) * sizeof(double); }
static size_t kde_mom_bytes() { return static_cast<size_t>(kKdeMomBlocks) * kKdeMomStride * sizeof(double); }

extern "C" size_t hm_kde_workspace_bytes(int64_t n_elems, int C, int m) {
    if (n_elems < 0 || C < 1 || m < 0) return 0;
    const size_t e = kde_eval_bytes(n_elems / C, m), mo = kde_mom_bytes();
    return e > mo ? e : mo;
}

extern "C" int hm_kde_moments(const double* val, const double* std, int64_t n_elems, int C, int channel, double* moments,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    const int rc = hm_rules::check_kde_moments(val, n_elems, C, channel, moments, workspace, workspace_bytes, true);
    if (rc != HM_OK) return rc;
    if (static_cast<size_t>(workspace_bytes) < kde_mom_bytes()) return HM_EINVAL;        // this build's own: the workspace's size
    const int64_t n = n_elems / C;
    double* part = static_cast<double*>(workspace);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_kde_moments1, dim3(kKdeMomBlocks), dim3(kKdeMomThreads), 0, st, val, std, n, C, channel, part);
    hipLaunchKernelGGL(k_kde_finish, dim3(1), dim3(kWave), 0, st, part, kMom1, 0, moments);
    hipLaunchKernelGGL(k_kde_moments2, dim3(kKdeMomBlocks), dim3(kKdeMomThreads), 0, st, val, std, n, C, channel,
                       static_cast<const double*>(moments), part);
    hipLaunchKernelGGL(k_kde_finish, dim3(1), dim3(kWave), 0, st, part, 1, 10, moments);
    return launch_status();
}

extern "C" int hm_kde_evaluate(const double* val, const double* std, int64_t n_elems, int C, int channel, double h, double scale,
                               const double* grid, int m, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
    bool empty;
    const int rc = hm_rules::check_kde_evaluate(val, n_elems, C, channel, h, scale, grid, m, out, workspace, workspace_bytes, true, empty);
    if (rc != HM_OK || empty) return rc;
    const int64_t n = n_elems / C;
    if (static_cast<size_t>(workspace_bytes) < kde_eval_bytes(n, m)) return HM_EINVAL;   // this build's own: the workspace's size
    const int64_t chunks = kde_chunks(n);
    double* part = static_cast<double*>(workspace);
    hipStream_t st = as_stream(stream);
    const unsigned gb = static_cast<unsigned>((static_cast<int64_t>(m) + kKdeBlockPts - 1) / kKdeBlockPts);
    hipLaunchKernelGGL(k_kde_eval, dim3(gb, static_cast<unsigned>(chunks)), dim3(kKdeBlock), 0, st, val, std, n, C, channel, h, grid, m,
                       kde_chunk_len(n), part);
    const unsigned gs = static_cast<unsigned>((static_cast<int64_t>(m) + kKdeSumJ - 1) / kKdeSumJ);
    hipLaunchKernelGGL(k_kde_sum, dim3(gs), dim3(kKdeSumJ * kKdeSumS), 0, st, static_cast<const double*>(part), chunks, m, scale, out);
    return launch_status();
}
