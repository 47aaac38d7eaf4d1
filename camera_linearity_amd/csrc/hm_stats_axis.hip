// hm_stats_axis.hip - statistics over any axis as HIP kernels (gfx950): hm_axis_statistics, hm_axis_statistics2 and their _workspace_bytes.
// compute_dimension_statistics over ANY axis (modules/measurand.py:318-350 take a NumPy axis argument): the array is seen as a dense
// (outer, A, inner) block and reduced over A - out[o, i] from x[(o A + k) inner + i], k = 0..A-1. (Two separate groups of reduced axes:
// hm_axis_statistics2 / k_axis_final2 below; three or more are brought together by the caller with a layout copy.) Same one-pass moments and NaN rules as the channel statistics
// (hm_moments.h: MomAcc / mom_merge / mom_finish). Two shapes:
//   k_axis_thread   one thread per output (o, i): lanes run along i (contiguous) - inner >= 16, or short axes (A <= 32: e.g. the
//                   channel axis of an image, where a lane reads its A consecutive values itself);
//   k_axis_row      inner < 16 and a long axis: the A x inner values of one o are contiguous; a workgroup strides over them with a
//                   thread count that is a multiple of inner (every thread keeps ONE channel), then folds threads of equal channel.
// Both split A into KS segments (grid dimension) when there are too few outputs to fill the chip; k_axis_final folds the segments.
#include "hm_moments.h"
#include "hm_rules_common.h"

namespace hm {

__device__ __forceinline__ void axis_finish_store(const Mom& m, bool weighted, int64_t j, double* out_mean, double* out_std, double* out_err) {
    double mean, sdv, err;
    mom_finish(m, weighted, mean, sdv, err);
    out_mean[j] = mean; out_std[j] = sdv;
    if (out_err) out_err[j] = err;
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_axis_thread(const double* __restrict__ val, const double* __restrict__ sd, int64_t outer, int64_t A,
                                                     int64_t inner, int KS, double* __restrict__ partial, double* __restrict__ out_mean,
                                                     double* __restrict__ out_std, double* __restrict__ out_err, int keep_partial) {
    const int64_t n_out = outer * inner;
    const int seg = blockIdx.y;
    const int64_t jstride = static_cast<int64_t>(gridDim.x) * 256;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; j < n_out; j += jstride) {
        const int64_t o = j / inner, i = j - o * inner;
        const double* pv = val + (o * A) * inner + i;
        const double* ps = WEIGHTED ? sd + (o * A) * inner + i : nullptr;
        MomAcc st = acc_zero();
        int it = 0;
        // four axis positions per iteration, their loads issued together (one dependent load per iteration left the lanes waiting on HBM
        // latency: 0.36 of the roofline on axis 0 of a 4096 x 4096 x 3 image)
        constexpr int UNR = 4;
        int64_t k = seg;
        for (; k + static_cast<int64_t>(UNR - 1) * KS < A; k += static_cast<int64_t>(UNR) * KS) {
            double v[UNR], sv[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                v[u] = __builtin_nontemporal_load(pv + (k + static_cast<int64_t>(u) * KS) * inner);
                sv[u] = WEIGHTED ? __builtin_nontemporal_load(ps + (k + static_cast<int64_t>(u) * KS) * inner) : 1.0;
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const double w = WEIGHTED ? 1.0 / sv[u] : 1.0;                  // measurand.py:342
                acc_add(st, v[u], w, sv[u], WEIGHTED, true);
            }
            it += UNR;
            if ((it & (kMomBlock - 1)) == 0 || it == UNR) acc_fold<false>(st);
        }
        if (k < A) {                                                            // the last 1-3 positions: loads together, missing ones at weight 0
            double v[UNR - 1], sv[UNR - 1];
            bool ok[UNR - 1];
#pragma unroll
            for (int u = 0; u < UNR - 1; ++u) {
                const int64_t kk = k + static_cast<int64_t>(u) * KS;
                ok[u] = kk < A;
                const int64_t kc = ok[u] ? kk : k;
                v[u] = pv[kc * inner];
                sv[u] = WEIGHTED ? ps[kc * inner] : 1.0;
            }
#pragma unroll
            for (int u = 0; u < UNR - 1; ++u) {
                const double w = WEIGHTED ? 1.0 / sv[u] : 1.0;
                acc_add(st, v[u], w, sv[u], WEIGHTED, ok[u]);
            }
        }
        const Mom m = acc_finish<false>(st, WEIGHTED);
        if (KS == 1 && !keep_partial) axis_finish_store(m, WEIGHTED, j, out_mean, out_std, out_err);
        else mom_store(partial + (static_cast<int64_t>(seg) * n_out + j) * kMomVals, m);
    }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_axis_row(const double* __restrict__ val, const double* __restrict__ sd, int64_t outer, int64_t A,
                                                  int64_t inner, int KS, double* __restrict__ partial, double* __restrict__ out_mean,
                                                  double* __restrict__ out_std, double* __restrict__ out_err, int keep_partial) {
    __shared__ double red[256][kMomVals];
    const int in = static_cast<int>(inner);
    const int Tm = (256 / in) * in;                                             // active threads: a multiple of inner
    const int seg = blockIdx.x;
    const int64_t seg_k = (A + KS - 1) / KS;                                    // axis positions per segment
    const int64_t e_lo = static_cast<int64_t>(seg) * seg_k * inner;
    int64_t e_hi = e_lo + seg_k * inner;
    if (e_hi > A * inner) e_hi = A * inner;
    const int64_t n_out = outer * inner;
    for (int64_t o = blockIdx.y; o < outer; o += gridDim.y) {
        MomAcc st = acc_zero();
        if (static_cast<int>(threadIdx.x) < Tm) {
            const double* pv = val + o * A * inner;
            const double* ps = WEIGHTED ? sd + o * A * inner : nullptr;
            int it = 0;
            constexpr int UNR = 4;
            int64_t e = e_lo + threadIdx.x;
            for (; e + static_cast<int64_t>(UNR - 1) * Tm < e_hi; e += static_cast<int64_t>(UNR) * Tm) {
                double v[UNR], sv[UNR];
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    v[u] = __builtin_nontemporal_load(pv + e + static_cast<int64_t>(u) * Tm);
                    sv[u] = WEIGHTED ? __builtin_nontemporal_load(ps + e + static_cast<int64_t>(u) * Tm) : 1.0;
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    const double w = WEIGHTED ? 1.0 / sv[u] : 1.0;
                    acc_add(st, v[u], w, sv[u], WEIGHTED, true);
                }
                it += UNR;
                if ((it & (kMomBlock - 1)) == 0 || it == UNR) acc_fold<false>(st);
            }
            for (; e < e_hi; e += Tm) {
                const double v = pv[e];
                const double s = WEIGHTED ? ps[e] : 1.0;
                const double w = WEIGHTED ? 1.0 / s : 1.0;
                acc_add(st, v, w, s, WEIGHTED, true);
                if ((++it & (kMomBlock - 1)) == 0) acc_fold<false>(st);
            }
        }
        const Mom mine = acc_finish<false>(st, WEIGHTED);
        __syncthreads();                                                        // (the previous o is done with `red`)
        mom_store(red[threadIdx.x], mine);
        __syncthreads();
        // thread t = p * inner + c holds partial p of channel c: a halving tree over p (fixed order; 7 steps for 85 partials - the serial fold
        // by `inner` threads it replaces was 85 dependent divisions per row)
        for (int P = Tm / in; P > 1; P = (P + 1) / 2) {
            const int half = (P + 1) / 2;
            const int pidx = static_cast<int>(threadIdx.x) / in;
            const bool act = static_cast<int>(threadIdx.x) < Tm && pidx < half && pidx + half < P;
            Mom r = mom_zero();
            if (act) r = mom_merge(mom_load(red[threadIdx.x]), mom_load(red[threadIdx.x + half * in]));
            __syncthreads();
            if (act) mom_store(red[threadIdx.x], r);
            __syncthreads();
        }
        if (static_cast<int>(threadIdx.x) < in) {
            const Mom m = mom_load(red[threadIdx.x]);
            const int64_t j = o * inner + threadIdx.x;
            if (KS == 1 && !keep_partial) axis_finish_store(m, WEIGHTED, j, out_mean, out_std, out_err);
            else mom_store(partial + (static_cast<int64_t>(seg) * n_out + j) * kMomVals, m);
        }
    }
}

__global__ __launch_bounds__(256) void k_axis_final(const double* __restrict__ partial, int KS, int64_t n_out, int weighted,
                                                    double* __restrict__ out_mean, double* __restrict__ out_std, double* __restrict__ out_err) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; j < n_out; j += stride) {
        Mom m = mom_load(partial + j * kMomVals);
        for (int s = 1; s < KS; ++s) m = mom_merge(m, mom_load(partial + (static_cast<int64_t>(s) * n_out + j) * kMomVals));
        axis_finish_store(m, weighted != 0, j, out_mean, out_std, out_err);
    }
}

// few outputs, many segments: one workgroup per output, thread t folds segments t, t + 256, ... and an LDS tree finishes (a single thread
// folding 1024 segments one after the other took 50 us)
__global__ __launch_bounds__(256) void k_axis_final_tree(const double* __restrict__ partial, int KS, int64_t n_out, int weighted,
                                                         double* __restrict__ out_mean, double* __restrict__ out_std, double* __restrict__ out_err) {
    __shared__ double tree[256][kMomVals];
    const int64_t j = blockIdx.x;
    Mom m = mom_zero();
    for (int s = threadIdx.x; s < KS; s += 256) m = mom_merge(m, mom_load(partial + (static_cast<int64_t>(s) * n_out + j) * kMomVals));
    mom_store(tree[threadIdx.x], m);
    __syncthreads();
    for (int span = 128; span > 0; span >>= 1) {
        if (static_cast<int>(threadIdx.x) < span) {
            const Mom r = mom_merge(mom_load(tree[threadIdx.x]), mom_load(tree[threadIdx.x + span]));
            mom_store(tree[threadIdx.x], r);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) axis_finish_store(mom_load(tree[0]), weighted != 0, j, out_mean, out_std, out_err);
}

// Two groups of reduced axes with kept axes between them - the array as (outer, A1, mid, A2, inner), reduced over A1 and A2 with no layout
// copy of the input. Stage 1 is the one-group reduction over the LONGER of the two (A1: inner' = mid * A2 * inner; A2: outer' = outer * A1 *
// mid), its states kept as partials; stage 2 folds, per output (o, m, i), the R positions of the other group and the KS segments in a fixed
// order: state index o * o_stride + m * m_stride + r * r_stride + i.
struct Final2K { int64_t n_out1, n_out2, mid, inner, o_stride, m_stride, r_stride, R; int KS, weighted; };
__device__ __forceinline__ int64_t final2_base(const Final2K& f, int64_t j) {
    const int64_t i = j % f.inner, om = j / f.inner;
    return (om / f.mid) * f.o_stride + (om % f.mid) * f.m_stride + i;
}
__global__ __launch_bounds__(256) void k_axis_final2(const double* __restrict__ partial, const Final2K f, double* __restrict__ out_mean,
                                                     double* __restrict__ out_std, double* __restrict__ out_err) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    for (int64_t j = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; j < f.n_out2; j += stride) {
        const int64_t base = final2_base(f, j);
        Mom m = mom_zero();
        for (int64_t r = 0; r < f.R; ++r)
            for (int s = 0; s < f.KS; ++s) m = mom_merge(m, mom_load(partial + (static_cast<int64_t>(s) * f.n_out1 + base + r * f.r_stride) * kMomVals));
        axis_finish_store(m, f.weighted != 0, j, out_mean, out_std, out_err);
    }
}
// few outputs, many states each: one workgroup per output, thread t folds states t, t + 256, ... of the R x KS, then an LDS tree
__global__ __launch_bounds__(256) void k_axis_final2_tree(const double* __restrict__ partial, const Final2K f, double* __restrict__ out_mean,
                                                          double* __restrict__ out_std, double* __restrict__ out_err) {
    __shared__ double tree[256][kMomVals];
    const int64_t j = blockIdx.x, base = final2_base(f, j), total = f.R * f.KS;
    Mom m = mom_zero();
    for (int64_t q = threadIdx.x; q < total; q += 256) {
        const int64_t r = q / f.KS, sgm = q % f.KS;
        m = mom_merge(m, mom_load(partial + (sgm * f.n_out1 + base + r * f.r_stride) * kMomVals));
    }
    mom_store(tree[threadIdx.x], m);
    __syncthreads();
    for (int span = 128; span > 0; span >>= 1) {
        if (static_cast<int>(threadIdx.x) < span) {
            const Mom r = mom_merge(mom_load(tree[threadIdx.x]), mom_load(tree[threadIdx.x + span]));
            mom_store(tree[threadIdx.x], r);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) axis_finish_store(mom_load(tree[0]), f.weighted != 0, j, out_mean, out_std, out_err);
}

struct AxisPlan { bool row; int KS; };
static AxisPlan axis_plan(int64_t outer, int64_t A, int64_t inner) {
    AxisPlan p;
    p.row = inner < 16 && A > 32;
    int64_t ks = 1;
    if (!p.row) {
        const int64_t blocks = (outer * inner + 255) / 256;
        if (blocks < 1024) { ks = (1024 + blocks - 1) / blocks; const int64_t cap = A / 16 > 1 ? A / 16 : 1; if (ks > cap) ks = cap; }
        if (ks > 256) ks = 256;
    } else {
        const int64_t tm = (256 / inner) * inner;
        if (outer < 1024) { ks = (1024 + outer - 1) / outer; const int64_t cap = (A * inner) / (tm * 8) > 1 ? (A * inner) / (tm * 8) : 1; if (ks > cap) ks = cap; }
        if (ks > 1024) ks = 1024;
    }
    p.KS = static_cast<int>(ks);
    return p;
}

// stage 1 of both entry points: the one-group reduction; keep_partial = leave the states in `partial` even when there is one segment
static void launch_axis_stage1(const double* val, const double* std, int64_t outer, int64_t axis_len, int64_t inner, const AxisPlan& p,
                               double* partial, double* out_mean, double* out_std, double* out_err, int keep_partial, hipStream_t st) {
    const int64_t n_out = outer * inner;
    if (!p.row) {
        int64_t gx = (n_out + 255) / 256;
        if (gx > (int64_t{1} << 20)) gx = int64_t{1} << 20;
        const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(p.KS));
        if (std) hipLaunchKernelGGL(k_axis_thread<true>, grid, dim3(256), 0, st, val, std, outer, axis_len, inner, p.KS, partial, out_mean, out_std, out_err, keep_partial);
        else hipLaunchKernelGGL(k_axis_thread<false>, grid, dim3(256), 0, st, val, std, outer, axis_len, inner, p.KS, partial, out_mean, out_std, out_err, keep_partial);
    } else {
        const dim3 grid(static_cast<unsigned>(p.KS), static_cast<unsigned>(outer < 65535 ? outer : 65535));
        if (std) hipLaunchKernelGGL(k_axis_row<true>, grid, dim3(256), 0, st, val, std, outer, axis_len, inner, p.KS, partial, out_mean, out_std, out_err, keep_partial);
        else hipLaunchKernelGGL(k_axis_row<false>, grid, dim3(256), 0, st, val, std, outer, axis_len, inner, p.KS, partial, out_mean, out_std, out_err, keep_partial);
    }
}

// which group stage 1 reduces (the longer one), the (outer, A, inner) view it sees and the index map of stage 2
struct Axis2Plan { int64_t outer1, A, inner1; AxisPlan p; Final2K f; };
static Axis2Plan axis2_plan(int64_t outer, int64_t a1, int64_t mid, int64_t a2, int64_t inner) {
    Axis2Plan q{};
    if (a1 >= a2) {            // stage 1 over A1: state index ((o mid + m) A2 + r) inner + i
        q.outer1 = outer; q.A = a1; q.inner1 = mid * a2 * inner;
        q.f.o_stride = mid * a2 * inner; q.f.m_stride = a2 * inner; q.f.r_stride = inner; q.f.R = a2;
    } else {                   // stage 1 over A2: state index ((o A1 + r) mid + m) inner + i
        q.outer1 = outer * a1 * mid; q.A = a2; q.inner1 = inner;
        q.f.o_stride = a1 * mid * inner; q.f.m_stride = inner; q.f.r_stride = mid * inner; q.f.R = a1;
    }
    q.p = axis_plan(q.outer1, q.A, q.inner1);
    q.f.n_out1 = q.outer1 * q.inner1; q.f.n_out2 = outer * mid * inner; q.f.mid = mid; q.f.inner = inner; q.f.KS = q.p.KS;
    return q;
}

}  // namespace hm

extern "C" size_t hm_axis_statistics_workspace_bytes(int64_t outer, int64_t axis_len, int64_t inner) {
    if (hm_rules::dense_elems({outer, axis_len, inner}) < 0) return 0;
    const hm::AxisPlan p = hm::axis_plan(outer, axis_len, inner);
    return p.KS > 1 ? static_cast<size_t>(p.KS) * static_cast<size_t>(outer * inner) * hm::kMomVals * sizeof(double) : 0;
}

extern "C" int hm_axis_statistics(const double* val, const double* std, int64_t outer, int64_t axis_len, int64_t inner,
                                  double* out_mean, double* out_std, double* out_err, void* workspace, void* stream) {
    using namespace hm;
    if (hm_rules::dense_elems({outer, axis_len, inner}) < 0 || !val || !out_mean || !out_std) return HM_EINVAL;
    if (!aligned(val, 8) || (std && !aligned(std, 8))) return HM_EALIGN;
    const AxisPlan p = axis_plan(outer, axis_len, inner);
    if (p.KS > 1 && !workspace) return HM_EINVAL;
    double* partial = static_cast<double*>(workspace);
    hipStream_t st = as_stream(stream);
    const int64_t n_out = outer * inner;
    launch_axis_stage1(val, std, outer, axis_len, inner, p, partial, out_mean, out_std, out_err, 0, st);
    if (p.KS > 1) {
        if (p.KS >= 32 && n_out <= 4096)
            hipLaunchKernelGGL(k_axis_final_tree, dim3(static_cast<unsigned>(n_out)), dim3(256), 0, st, partial, p.KS, n_out, std ? 1 : 0, out_mean, out_std, out_err);
        else
            hipLaunchKernelGGL(k_axis_final, dim3(stream_grid(n_out, 256, 8)), dim3(256), 0, st, partial, p.KS, n_out, std ? 1 : 0, out_mean, out_std, out_err);
    }
    return launch_status();
}

extern "C" size_t hm_axis_statistics2_workspace_bytes(int64_t outer, int64_t a1, int64_t mid, int64_t a2, int64_t inner) {
    if (hm_rules::dense_elems({outer, a1, mid, a2, inner}) < 0) return 0;
    const hm::Axis2Plan q = hm::axis2_plan(outer, a1, mid, a2, inner);
    return static_cast<size_t>(q.p.KS) * static_cast<size_t>(q.f.n_out1) * hm::kMomVals * sizeof(double);
}

extern "C" int hm_axis_statistics2(const double* val, const double* std, int64_t outer, int64_t a1, int64_t mid, int64_t a2, int64_t inner,
                                   double* out_mean, double* out_std, double* out_err, void* workspace, void* stream) {
    using namespace hm;
    if (hm_rules::dense_elems({outer, a1, mid, a2, inner}) < 0 || !val || !out_mean || !out_std || !workspace) return HM_EINVAL;
    if (!aligned(val, 8) || (std && !aligned(std, 8))) return HM_EALIGN;
    Axis2Plan q = axis2_plan(outer, a1, mid, a2, inner);
    q.f.weighted = std ? 1 : 0;
    double* partial = static_cast<double*>(workspace);
    hipStream_t st = as_stream(stream);
    launch_axis_stage1(val, std, q.outer1, q.A, q.inner1, q.p, partial, nullptr, nullptr, nullptr, 1, st);
    if (q.f.R * q.f.KS >= 64 && q.f.n_out2 <= 4096)
        hipLaunchKernelGGL(k_axis_final2_tree, dim3(static_cast<unsigned>(q.f.n_out2)), dim3(256), 0, st, partial, q.f, out_mean, out_std, out_err);
    else
        hipLaunchKernelGGL(k_axis_final2, dim3(stream_grid(q.f.n_out2, 256, 8)), dim3(256), 0, st, partial, q.f, out_mean, out_std, out_err);
    return launch_status();
}
