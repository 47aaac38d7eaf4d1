// hm_pointwise.hip - the element-wise operators of the linearity-statistics row of SURVEY.md 8(f)-1 as HIP kernels (gfx950):
//   hm_apply_thresholds      AbstractMeasurand.apply_thresholds          modules/measurand.py:375-428
//   hm_compute_difference    AbstractMeasurand.compute_difference        modules/measurand.py:620-655
//   hm_interpolate           AbstractMeasurand.interpolate               modules/measurand.py:657-681
//   hm_compute_difference_bcast, hm_interpolate_bcast    the same two on broadcast operands   modules/measurand.py:621-681
// Streaming, HBM-bound. The statistics of the row: hm_stats.hip, hm_stats_hist.hip, hm_stats_axis.hip.
#include "hm_pointwise.h"
#include "hm_ops_math.h"
#include "hm_ops_rules.h"

namespace hm {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// In place; two elements per lane (16-byte loads; a store only where something changes - thresholds usually clip a
// minority), running channel counter.
__global__ __launch_bounds__(256) void k_thresholds(double* __restrict__ val, double* __restrict__ sd, const ChanLimits lim,
                                                    int64_t n, int C) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int64_t units = n / 2;
    const bool vec_ok = aligned_dev(val, 16) && (!sd || aligned_dev(sd, 16));
    const uint32_t uC = static_cast<uint32_t>(C);
    const int64_t u0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    uint32_t c0 = static_cast<uint32_t>((2 * u0) % C);
    const uint32_t cstep = static_cast<uint32_t>((2 * stride) % C);
    auto lo_of = [&](uint32_t c) { double r = lim.lo[0]; for (int k = 1; k < HM_MAX_CHANNELS; ++k) r = c == static_cast<uint32_t>(k) ? lim.lo[k] : r; return r; };
    auto hi_of = [&](uint32_t c) { double r = lim.hi[0]; for (int k = 1; k < HM_MAX_CHANNELS; ++k) r = c == static_cast<uint32_t>(k) ? lim.hi[k] : r; return r; };
    for (int64_t u = u0; u < units; u += stride) {
        const int64_t e = 2 * u;
        const uint32_t c1 = c0 + 1u == uC ? 0u : c0 + 1u;
        double v0, v1;
        if (vec_ok) { const f64x2 a = *reinterpret_cast<const f64x2*>(val + e); v0 = a.x; v1 = a.y; }
        else { v0 = val[e]; v1 = val[e + 1]; }
        const bool k0 = (v0 < lo_of(c0)) || (v0 > hi_of(c0));           // measurand.py:418 (NaN compares false: stays NaN)
        const bool k1 = (v1 < lo_of(c1)) || (v1 > hi_of(c1));
        if (k0) { val[e] = nan; if (sd) sd[e] = nan; }
        if (k1) { val[e + 1] = nan; if (sd) sd[e + 1] = nan; }
        c0 += cstep;
        if (c0 >= uC) c0 -= uC;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) {
        const int64_t e = n - 1;
        const uint32_t c = static_cast<uint32_t>(e % C);
        const double v = val[e];
        if ((v < lo_of(c)) || (v > hi_of(c))) { val[e] = nan; if (sd) sd[e] = nan; }
    }
}

__global__ __launch_bounds__(256) void k_difference(const double* __restrict__ x, const double* __restrict__ sx,
                                                    const double* __restrict__ y, const double* __restrict__ sy, double mult,
                                                    double* __restrict__ ad, double* __restrict__ ads,
                                                    double* __restrict__ rd, double* __restrict__ rds, int64_t n) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += stride) {
        const double xv = x[e], yv = y[e];
        const double a = diff_abs(xv, yv, mult);
        ad[e] = a;
        rd[e] = diff_rel(a, yv, mult);
        if (ads) {
            const double xs = sx ? sx[e] : 0.0, ys = sy ? sy[e] : 0.0;
            ads[e] = diff_abs_std(xs, ys, mult);
            rds[e] = diff_rel_std(xv, yv, xs, ys, mult);
        }
    }
}

// dense, 16-byte-aligned buffers: two elements per lane, 16-byte nontemporal accesses, std presence at compile time (the
// per-element kernel above measured 0.63 of 8 TB/s on its eight streams)
template <bool SX, bool SY>
__global__ __launch_bounds__(256) void k_difference_dense(const double* __restrict__ x, const double* __restrict__ sx,
                                                          const double* __restrict__ y, const double* __restrict__ sy, double mult,
                                                          double* __restrict__ ad, double* __restrict__ ads,
                                                          double* __restrict__ rd, double* __restrict__ rds, int64_t n) {
    constexpr bool STD = SX || SY;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t pairs = n / 2;
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < pairs; q += stride) {
        const f64x2 xv = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(x) + q);
        const f64x2 yv = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(y) + q);
        f64x2 xs = {0.0, 0.0}, ys = {0.0, 0.0};
        if constexpr (SX) xs = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(sx) + q);
        if constexpr (SY) ys = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(sy) + q);
        double a0, a1, r0, r1, as0 = 0.0, as1 = 0.0, rs0 = 0.0, rs1 = 0.0;
        diff_terms(xv.x, yv.x, xs.x, ys.x, mult, STD, a0, r0, as0, rs0);
        diff_terms(xv.y, yv.y, xs.y, ys.y, mult, STD, a1, r1, as1, rs1);
        f64x2 o;
        o.x = a0; o.y = a1; __builtin_nontemporal_store(o, reinterpret_cast<f64x2*>(ad) + q);
        o.x = r0; o.y = r1; __builtin_nontemporal_store(o, reinterpret_cast<f64x2*>(rd) + q);
        if constexpr (STD) {
            o.x = as0; o.y = as1; __builtin_nontemporal_store(o, reinterpret_cast<f64x2*>(ads) + q);
            o.x = rs0; o.y = rs1; __builtin_nontemporal_store(o, reinterpret_cast<f64x2*>(rds) + q);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t e = n - 1;
        double a, r, as = 0.0, rs = 0.0;
        diff_terms(x[e], y[e], SX ? sx[e] : 0.0, SY ? sy[e] : 0.0, mult, STD, a, r, as, rs);
        ad[e] = a; rd[e] = r;
        if constexpr (STD) { ads[e] = as; rds[e] = rs; }
    }
}

// the burst access shape (hm_ops.hip: k_binary_burst; tools/readbench.hip copysweep): a wave owns chunks of 512 elements, issues the four
// 16-byte loads per lane of every input stream back to back, then the stores of every output stream. Whole chunks only.
constexpr int kDiffBurst = 4;
constexpr int64_t kDiffChunk = 128 * kDiffBurst;
template <bool SX, bool SY>
__global__ __launch_bounds__(256) void k_difference_burst(const double* __restrict__ x, const double* __restrict__ sx,
                                                          const double* __restrict__ y, const double* __restrict__ sy, double mult,
                                                          double* __restrict__ ad, double* __restrict__ ads,
                                                          double* __restrict__ rd, double* __restrict__ rds, int64_t n_chunks) {
    constexpr bool STD = SX || SY;
    constexpr int B = kDiffBurst;
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t cstride = static_cast<int64_t>(gridDim.x) * 4;
    for (int64_t c = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); c < n_chunks; c += cstride) {
        const int64_t b = c * kDiffChunk;
        f64x2 xv[B], yv[B], xs[B], ys[B];
#pragma unroll
        for (int k = 0; k < B; ++k) xv[k] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(x + b + 128 * k) + lane);
#pragma unroll
        for (int k = 0; k < B; ++k) yv[k] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(y + b + 128 * k) + lane);
#pragma unroll
        for (int k = 0; k < B; ++k) {
            xs[k] = f64x2{0.0, 0.0};
            if constexpr (SX) xs[k] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(sx + b + 128 * k) + lane);
        }
#pragma unroll
        for (int k = 0; k < B; ++k) {
            ys[k] = f64x2{0.0, 0.0};
            if constexpr (SY) ys[k] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(sy + b + 128 * k) + lane);
        }
        f64x2 a[B], r[B], as[B], rs[B];
#pragma unroll
        for (int k = 0; k < B; ++k) {
            double a0, a1, r0, r1, as0 = 0.0, as1 = 0.0, rs0 = 0.0, rs1 = 0.0;
            diff_terms(xv[k].x, yv[k].x, xs[k].x, ys[k].x, mult, STD, a0, r0, as0, rs0);
            diff_terms(xv[k].y, yv[k].y, xs[k].y, ys[k].y, mult, STD, a1, r1, as1, rs1);
            a[k] = f64x2{a0, a1}; r[k] = f64x2{r0, r1}; as[k] = f64x2{as0, as1}; rs[k] = f64x2{rs0, rs1};
        }
#pragma unroll
        for (int k = 0; k < B; ++k) __builtin_nontemporal_store(a[k], reinterpret_cast<f64x2*>(ad + b + 128 * k) + lane);
#pragma unroll
        for (int k = 0; k < B; ++k) __builtin_nontemporal_store(r[k], reinterpret_cast<f64x2*>(rd + b + 128 * k) + lane);
        if constexpr (STD) {
#pragma unroll
            for (int k = 0; k < B; ++k) __builtin_nontemporal_store(as[k], reinterpret_cast<f64x2*>(ads + b + 128 * k) + lane);
#pragma unroll
            for (int k = 0; k < B; ++k) __builtin_nontemporal_store(rs[k], reinterpret_cast<f64x2*>(rds + b + 128 * k) + lane);
        }
    }
}

__global__ __launch_bounds__(256) void k_interpolate(const double* __restrict__ x0, const double* __restrict__ s0,
                                                     const double* __restrict__ x1, const double* __restrict__ s1,
                                                     double y0, double y1, double y, double* __restrict__ out,
                                                     double* __restrict__ out_std, int64_t n) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const InterpCoef k = interp_coef(y0, y1, y);
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += stride) {
        out[e] = interp_value(k, x0[e], x1[e]);
        if (out_std) out_std[e] = interp_std(k, s0 ? s0[e] : 0.0, s1 ? s1[e] : 0.0);
    }
}

// interpolate in the burst access shape (k_difference_burst): whole 512-element chunks of 16-byte aligned, dense buffers
template <bool S0, bool S1>
__global__ __launch_bounds__(256) void k_interpolate_burst(const double* __restrict__ x0, const double* __restrict__ s0,
                                                           const double* __restrict__ x1, const double* __restrict__ s1,
                                                           double y0, double y1, double y, double* __restrict__ out,
                                                           double* __restrict__ out_std, int64_t n_chunks) {
    constexpr bool STD = S0 || S1;
    constexpr int B = kDiffBurst;
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t cstride = static_cast<int64_t>(gridDim.x) * 4;
    const InterpCoef ic = interp_coef(y0, y1, y);
    for (int64_t c = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); c < n_chunks; c += cstride) {
        const int64_t e = c * kDiffChunk;
        f64x2 v0[B], v1[B], u0[B], u1[B];
#pragma unroll
        for (int k = 0; k < B; ++k) v0[k] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(x0 + e + 128 * k) + lane);
#pragma unroll
        for (int k = 0; k < B; ++k) v1[k] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(x1 + e + 128 * k) + lane);
#pragma unroll
        for (int k = 0; k < B; ++k) {
            u0[k] = f64x2{0.0, 0.0};
            if constexpr (S0) u0[k] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(s0 + e + 128 * k) + lane);
        }
#pragma unroll
        for (int k = 0; k < B; ++k) {
            u1[k] = f64x2{0.0, 0.0};
            if constexpr (S1) u1[k] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(s1 + e + 128 * k) + lane);
        }
        f64x2 o[B], os[B];
#pragma unroll
        for (int k = 0; k < B; ++k) {
            o[k] = f64x2{interp_value(ic, v0[k].x, v1[k].x), interp_value(ic, v0[k].y, v1[k].y)};
            os[k] = f64x2{interp_std(ic, u0[k].x, u1[k].x), interp_std(ic, u0[k].y, u1[k].y)};
        }
#pragma unroll
        for (int k = 0; k < B; ++k) __builtin_nontemporal_store(o[k], reinterpret_cast<f64x2*>(out + e + 128 * k) + lane);
        if constexpr (STD) {
#pragma unroll
            for (int k = 0; k < B; ++k) __builtin_nontemporal_store(os[k], reinterpret_cast<f64x2*>(out_std + e + 128 * k) + lane);
        }
    }
}

// apply_thresholds for more than HM_MAX_CHANNELS channels on the last axis (the reference's property tests draw up to 10):
// limits staged in LDS (uniform loop over the kernarg arrays), one element per thread.
struct ChanLimitsWide { double lo[HM_THRESHOLD_MAX_CHANNELS]; double hi[HM_THRESHOLD_MAX_CHANNELS]; };
__global__ __launch_bounds__(256) void k_thresholds_wide(double* __restrict__ val, double* __restrict__ sd, const ChanLimitsWide lim,
                                                         int64_t n, int C) {
    __shared__ double lo[HM_THRESHOLD_MAX_CHANNELS], hi[HM_THRESHOLD_MAX_CHANNELS];
    for (int k = 0; k < C; ++k)
        if (threadIdx.x == 0) { lo[k] = lim.lo[k]; hi[k] = lim.hi[k]; }
    __syncthreads();
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += stride) {
        const int c = static_cast<int>(e % C);
        const double v = val[e];
        if ((v < lo[c]) || (v > hi[c])) { val[e] = nan; if (sd) sd[e] = nan; }       // measurand.py:418
    }
}

// compute_difference / interpolate on BROADCAST operands (modules/measurand.py:621-681 apply NumPy broadcasting to x and y): element
// strides with 0 on broadcast axes, as hm_binary_op; x and its std share strides (one Measurand), y and its std likewise.
struct Bcast2K { int64_t shape[HM_MAX_DIMS], st1[HM_MAX_DIMS], st2[HM_MAX_DIMS]; int ndim; };
__device__ __forceinline__ void bcast_offsets(const Bcast2K& b, int64_t e, int64_t& o1, int64_t& o2) {
    o1 = 0; o2 = 0;
    int64_t rem = e;
    for (int d = b.ndim - 1; d >= 0; --d) {
        const int64_t i = rem % b.shape[d];
        rem /= b.shape[d];
        o1 += i * b.st1[d];
        o2 += i * b.st2[d];
    }
}
__global__ __launch_bounds__(256) void k_difference_bcast(const double* __restrict__ x, const double* __restrict__ sx,
                                                          const double* __restrict__ y, const double* __restrict__ sy, double mult,
                                                          double* __restrict__ ad, double* __restrict__ ads,
                                                          double* __restrict__ rd, double* __restrict__ rds, int64_t n, const Bcast2K b) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += stride) {
        int64_t ox, oy;
        bcast_offsets(b, e, ox, oy);
        const double xv = x[ox], yv = y[oy];
        const double a = diff_abs(xv, yv, mult);
        ad[e] = a;
        rd[e] = diff_rel(a, yv, mult);
        if (ads) {
            const double xs = sx ? sx[ox] : 0.0, ys = sy ? sy[oy] : 0.0;
            ads[e] = diff_abs_std(xs, ys, mult);
            rds[e] = diff_rel_std(xv, yv, xs, ys, mult);
        }
    }
}
__global__ __launch_bounds__(256) void k_interpolate_bcast(const double* __restrict__ x0, const double* __restrict__ s0,
                                                           const double* __restrict__ x1, const double* __restrict__ s1,
                                                           double y0, double y1, double y, double* __restrict__ out,
                                                           double* __restrict__ out_std, int64_t n, const Bcast2K b) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const InterpCoef k = interp_coef(y0, y1, y);
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += stride) {
        int64_t o0, o1;
        bcast_offsets(b, e, o0, o1);
        out[e] = interp_value(k, x0[o0], x1[o1]);
        if (out_std) out_std[e] = interp_std(k, s0 ? s0[o0] : 0.0, s1 ? s1[o1] : 0.0);
    }
}

// the kernel argument of a checked broadcast (hm_rules::check_bcast)
static Bcast2K fill_bcast(int ndim, const int64_t* shape, const int64_t* st1, const int64_t* st2) {
    Bcast2K b;
    b.ndim = ndim;
    for (int d = 0; d < ndim; ++d) { b.shape[d] = shape[d]; b.st1[d] = st1[d]; b.st2[d] = st2[d]; }
    return b;
}

void launch_thresholds(double* val, double* sd, const ChanLimits& lim, int64_t n, int C, hipStream_t st) {
    hipLaunchKernelGGL(k_thresholds, dim3(stream_grid((n + 1) / 2, 256, 8)), dim3(256), 0, st, val, sd, lim, n, C);
}

}  // namespace hm

using namespace hm;

extern "C" int hm_apply_thresholds(double* val, double* std, const double* lower, const double* upper,
                                   int64_t n, int C, void* stream) {
    if (const int rc = hm_rules::check_apply_thresholds(val, std, lower, upper, n, C, hm_rules::DEVICE); rc != HM_OK || n == 0) return rc;
    if (C > HM_MAX_CHANNELS) {
        ChanLimitsWide w{};
        for (int c = 0; c < C; ++c) { w.lo[c] = lower[c]; w.hi[c] = upper[c]; }
        hipLaunchKernelGGL(k_thresholds_wide, dim3(stream_grid(n, 256, 8)), dim3(256), 0, as_stream(stream), val, std, w, n, C);
        return launch_status();
    }
    ChanLimits lim{};
    for (int c = 0; c < C; ++c) { lim.lo[c] = lower[c]; lim.hi[c] = upper[c]; }
    launch_thresholds(val, std, lim, n, C, as_stream(stream));
    return launch_status();
}

extern "C" int hm_compute_difference(const double* x, const double* sx, const double* y, const double* sy, double multiplier,
                                     double* out_abs, double* out_abs_std, double* out_rel, double* out_rel_std,
                                     int64_t n, void* stream) {
    int64_t one = 1, count;                 // checked as the _bcast form on shape {n}, strides {1}: n < 0 is its negative extent, n == 0 its "no element"
    if (const int rc = hm_rules::check_compute_difference_bcast(x, sx, y, sy, out_abs, out_abs_std, out_rel, out_rel_std, 1, &n, &one, &one, count);
        rc != HM_OK || n == 0) return rc;
    const bool with_std = sx || sy;
    const bool al16 = aligned(x, 16) && aligned(y, 16) && aligned(out_abs, 16) && aligned(out_rel, 16) && (!sx || aligned(sx, 16)) &&
                      (!sy || aligned(sy, 16)) && (!with_std || (aligned(out_abs_std, 16) && aligned(out_rel_std, 16)));
    if (al16) {
        const int64_t n_chunks = n / kDiffChunk;
        if (n_chunks > 0) {
            const unsigned bgrid = stream_grid((n_chunks + 3) / 4, 1, 16);
#define HM_DIFFB(A, B) hipLaunchKernelGGL((k_difference_burst<A, B>), dim3(bgrid), dim3(256), 0, as_stream(stream), \
                                          x, sx, y, sy, multiplier, out_abs, out_abs_std, out_rel, out_rel_std, n_chunks)
            if (sx && sy) HM_DIFFB(true, true); else if (sx) HM_DIFFB(true, false); else if (sy) HM_DIFFB(false, true); else HM_DIFFB(false, false);
#undef HM_DIFFB
            const int64_t done = n_chunks * kDiffChunk;                  // the remainder (< 512 elements) through the per-lane kernel
            if (done == n) return launch_status();
            x += done; y += done; out_abs += done; out_rel += done; n -= done;
            if (sx) sx += done;
            if (sy) sy += done;
            if (out_abs_std) { out_abs_std += done; out_rel_std += done; }
        }
        const unsigned dgrid = stream_grid((n + 1) / 2, 256, 8);
#define HM_DIFF(A, B) hipLaunchKernelGGL((k_difference_dense<A, B>), dim3(dgrid), dim3(256), 0, as_stream(stream), \
                                         x, sx, y, sy, multiplier, out_abs, out_abs_std, out_rel, out_rel_std, n)
        if (sx && sy) HM_DIFF(true, true); else if (sx) HM_DIFF(true, false); else if (sy) HM_DIFF(false, true); else HM_DIFF(false, false);
#undef HM_DIFF
        return launch_status();
    }
    hipLaunchKernelGGL(k_difference, dim3(stream_grid(n, 256, 8)), dim3(256), 0, as_stream(stream),
                       x, sx, y, sy, multiplier, out_abs, out_abs_std, out_rel, out_rel_std, n);
    return launch_status();
}

extern "C" int hm_interpolate(const double* x0, const double* s0, const double* x1, const double* s1,
                              double y0, double y1, double y, double* out, double* out_std, int64_t n, void* stream) {
    int64_t one = 1, count;                 // checked as the _bcast form on shape {n}, strides {1}: n < 0 is its negative extent, n == 0 its "no element"
    if (const int rc = hm_rules::check_interpolate_bcast(x0, s0, x1, s1, out, out_std, 1, &n, &one, &one, count); rc != HM_OK || n == 0) return rc;
    const bool al16 = aligned(x0, 16) && aligned(x1, 16) && aligned(out, 16) && (!s0 || aligned(s0, 16)) && (!s1 || aligned(s1, 16)) &&
                      (!out_std || aligned(out_std, 16));
    const int64_t n_chunks = n / kDiffChunk;
    if (al16 && n_chunks > 0) {
        const unsigned bgrid = stream_grid((n_chunks + 3) / 4, 1, 16);
#define HM_INTB(A, B) hipLaunchKernelGGL((k_interpolate_burst<A, B>), dim3(bgrid), dim3(256), 0, as_stream(stream), \
                                         x0, s0, x1, s1, y0, y1, y, out, out_std, n_chunks)
        if (s0 && s1) HM_INTB(true, true); else if (s0) HM_INTB(true, false); else if (s1) HM_INTB(false, true); else HM_INTB(false, false);
#undef HM_INTB
        const int64_t done = n_chunks * kDiffChunk;                      // the remainder (< 512 elements) through the per-lane kernel
        if (done == n) return launch_status();
        x0 += done; x1 += done; out += done; n -= done;
        if (s0) s0 += done;
        if (s1) s1 += done;
        if (out_std) out_std += done;
    }
    hipLaunchKernelGGL(k_interpolate, dim3(stream_grid(n, 256, 8)), dim3(256), 0, as_stream(stream),
                       x0, s0, x1, s1, y0, y1, y, out, out_std, n);
    return launch_status();
}

extern "C" int hm_compute_difference_bcast(const double* x, const double* sx, const double* y, const double* sy, double multiplier,
                                           double* out_abs, double* out_abs_std, double* out_rel, double* out_rel_std,
                                           int ndim, const int64_t* shape, const int64_t* strides_x, const int64_t* strides_y, void* stream) {
    int64_t n;
    if (const int rc = hm_rules::check_compute_difference_bcast(x, sx, y, sy, out_abs, out_abs_std, out_rel, out_rel_std, ndim, shape, strides_x,
                                                            strides_y, n); rc != HM_OK || n == 0) return rc;
    const hm::Bcast2K b = hm::fill_bcast(ndim, shape, strides_x, strides_y);
    hipLaunchKernelGGL(hm::k_difference_bcast, dim3(hm::stream_grid(n, 256, 8)), dim3(256), 0, hm::as_stream(stream),
                       x, sx, y, sy, multiplier, out_abs, out_abs_std, out_rel, out_rel_std, n, b);
    return hm::launch_status();
}

extern "C" int hm_interpolate_bcast(const double* x0, const double* s0, const double* x1, const double* s1, double y0, double y1, double y,
                                    double* out, double* out_std, int ndim, const int64_t* shape, const int64_t* strides0,
                                    const int64_t* strides1, void* stream) {
    int64_t n;
    if (const int rc = hm_rules::check_interpolate_bcast(x0, s0, x1, s1, out, out_std, ndim, shape, strides0, strides1, n); rc != HM_OK || n == 0) return rc;
    const hm::Bcast2K b = hm::fill_bcast(ndim, shape, strides0, strides1);
    hipLaunchKernelGGL(hm::k_interpolate_bcast, dim3(hm::stream_grid(n, 256, 8)), dim3(256), 0, hm::as_stream(stream),
                       x0, s0, x1, s1, y0, y1, y, out, out_std, n, b);
    return hm::launch_status();
}
