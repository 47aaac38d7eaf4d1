// hm_merge_hot.h - the fused merge's one-element-per-thread kernel and its hot-pixel pass (gfx950):
//   merge_generic                       anything the streaming kernels do not take (tails, unaligned tiles, variant < 0)
//   merge_fixup_hot                     the hot-pixel pass without a workspace: one hot element per wave at a time
//   merge_scan_hot + merge_patch_hot    the same pass through the hot-element queue in the caller's workspace
// with launch_generic / launch_fixup / launch_hot_queue. The kernel map of the whole merge is in hm_merge.hip. Nothing here is instantiated
// by including it: hm_merge_hot.hip instantiates the launchers for float64 std frames (with the val-only and table forms, and holds
// merge_scan_hot), hm_merge_hot_sd32.hip for float32 std frames (hm_merge_std_f32; template parameter SD = float).
#pragma once
#include "hm_merge_host.h"
#include "hm_merge_hot_scan.h"
#include <mutex>

namespace hm {

// ------------------------------------------------------------------------------------------------
// generic kernel: one element per thread, runtime N and C, uint8 or float64 frames.
// ------------------------------------------------------------------------------------------------
template <bool F64IN, bool STD, int OUT = OUT_F64, bool LUT = false, typename SD = double>
__global__ __launch_bounds__(256) void merge_generic(const MergeK a) {
    __shared__ double t_w[256], t_dw[256], t_g[256 * HM_MAX_CHANNELS], t_d[256 * HM_MAX_CHANNELS];
    reset_hot_counters(a);
    fill_plain_tables<F64IN, STD>(a, t_w, t_dw, t_g, t_d);
    __syncthreads();
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < a.n_elems; q += stride)
        merge_one_element<F64IN, STD, HOT_NONE, OUT, LUT, SD>(a, t_w, t_dw, t_g, t_d, a.elem0 + q, true);
}

// ------------------------------------------------------------------------------------------------
// hot-pixel fix-up.
// fixup_element(): one wave recomputes one output element `e` (wave-uniform) with the frames spread over
// the lanes - lane i < N owns frame i: its dark byte, its value and std are loaded in parallel (one memory
// latency instead of N); the k x k medians of ALL hot frames are taken at once by sub-groups of k*k lanes
// (floor(64 / k^2) frames per batch; ranks by ds_bpermute shuffles inside the sub-group); the per-frame
// terms are then formed in parallel and accumulated with readlane broadcasts IN FRAME ORDER, i.e. with
// exactly the operation sequence of merge_one_element(), so the fix-up is bit-identical to what a
// streaming kernel would have produced had it been given the filtered frames.
// ------------------------------------------------------------------------------------------------
// LUT (hm_merge_std_table): a frame's std, and every neighbour's, is the per-DN table entry of the value loaded beside it.
// SD (hm_merge_std_f32): element type of the std frames; a float std is widened as it is loaded (the median of the widened neighbourhood).
template <bool F64IN, bool STD, int OUT = OUT_F64, bool LUT = false, typename SD = double>
__device__ __forceinline__ void fixup_element(const MergeK& a, const double* t_w, const double* t_dw,
                                           const double* t_g, const double* t_d, int64_t e) {
    const int lane = threadIdx.x & 63;
    const int C = a.C, N = a.n_frames;
    const int64_t ei = a.in_off + e;
    const int c = static_cast<int>(e % C);
    int64_t row, col; int cc;
    elem_to_pixel(a, e, row, col, cc);
    const bool owner = lane < N;
    const int fi = owner ? lane : 0;
    // the lane's own frame: pointers picked with wave-uniform indices (a per-lane index into the kernarg
    // struct would make hipcc spill the whole struct to scratch for every thread of the kernel)
    const void* fr = a.frame[0];
    const SD* sp = a.template sd_as<SD>(0);
    const uint8_t* dk = a.dark[0];
    int dmin = a.dark_min[0];
    double it = a.inv_t[0];
    for (int i = 1; i < N; ++i) {
        const bool me = lane == i;
        fr = me ? a.frame[i] : fr;
        sp = me ? a.template sd_as<SD>(i) : sp;
        dk = me ? a.dark[i] : dk;
        dmin = me ? a.dark_min[i] : dmin;
        it = me ? a.inv_t[i] : it;
    }
    // --- parallel loads of the lane's own frame
    const bool hot = owner && dk && static_cast<int>(dk[ei]) >= dmin;
    double v = F64IN ? static_cast<const double*>(fr)[ei] : static_cast<double>(static_cast<const uint8_t*>(fr)[ei]);
    double sdv = 0.0;
    if constexpr (STD) sdv = LUT ? a.std_lut[(F64IN ? lut_index(v) : static_cast<uint32_t>(v)) * C + c] : static_cast<double>(sp[ei]);
    // --- medians of the hot frames, floor(64 / k^2) frames per batch
    const unsigned long long hotmask = __ballot(hot);
    const int k = a.median_k, kk = k * k, r = k / 2, m = kk / 2;
    const int B = 64 / kk;
    const int sub = lane / kk, p = lane % kk;
    for (int i0 = 0; i0 < N; i0 += B) {
        if (((hotmask >> i0) & ((B >= 64 ? ~0ull : ((1ull << B) - 1)))) == 0) continue;          // wave-uniform
        const int f = i0 + sub;
        const bool part = sub < B && f < N && ((hotmask >> f) & 1ull);
        const void* pf = a.frame[i0];
        const SD* ps = a.template sd_as<SD>(i0);
        for (int j = 1; j < B && i0 + j < N; ++j) {
            pf = sub == j ? a.frame[i0 + j] : pf;
            ps = sub == j ? a.template sd_as<SD>(i0 + j) : ps;
        }
        const int64_t yy = reflect_index(row + (p / k - r), a.H) - a.buf_row0;
        const int64_t xx = reflect_index(col + (p % k - r), a.W);
        const int64_t ni = (yy * a.W + xx) * C + cc;
        double nv = 0.0, ns = 0.0;
        if (part) {
            nv = F64IN ? static_cast<const double*>(pf)[ni] : static_cast<double>(static_cast<const uint8_t*>(pf)[ni]);
            if constexpr (STD) ns = LUT ? a.std_lut[(F64IN ? lut_index(nv) : static_cast<uint32_t>(nv)) * C + cc] : static_cast<double>(ps[ni]);
        }
        int lv = 0, qv = 0, ls = 0, qs = 0;
        for (int q = 0; q < kk; ++q) {
            const int src = sub * kk + q;
            const double uv = __shfl(nv, src, 64);
            lv += (uv < nv); qv += (uv <= nv);
            if (STD) { const double us = __shfl(ns, src, 64); ls += (us < ns); qs += (us <= ns); }
        }
        const unsigned long long medv = __ballot(part && lv <= m && m < qv);
        const unsigned long long meds = STD ? __ballot(part && ls <= m && m < qs) : 0ull;
        // owner lane of frame f picks the median out of its sub-group
        const int osub = fi - i0;
        const bool mine = hot && osub >= 0 && osub < B;
        const unsigned long long gmask = kk >= 64 ? ~0ull : ((1ull << kk) - 1);
        const int sh = mine ? osub * kk : 0;
        const unsigned long long gv = (medv >> sh) & gmask, gs = (meds >> sh) & gmask;
        const int srcv = sh + (gv ? __ffsll(static_cast<long long>(gv)) - 1 : 0);
        const int srcs = sh + (gs ? __ffsll(static_cast<long long>(gs)) - 1 : 0);
        const double mv = __shfl(nv, srcv, 64);
        const double ms = STD ? __shfl(ns, srcs, 64) : 0.0;
        if (mine) { v = mv; if (STD) sdv = ms; }
    }
    // --- per-frame quantities, in parallel
    double w = 0.0, dw = 0.0;
    uint32_t idx = 0;
    if (owner) {
        if (F64IN) {
            const double dv = v - 0.5;
            w = gauss_weight(dv);
            dw = gauss_dweight(dv, w);
            idx = lut_index(v);
        } else {
            idx = static_cast<uint32_t>(v);
            w = t_w[idx];
            dw = STD ? t_dw[idx] : 0.0;
        }
    }
    // --- S in frame order
    double S = 0.0;
    for (int i = 0; i < N; ++i) {
        const double wi = readlane_f64(w, i);
        S = (i == 0) ? wi : S + wi;
    }
    if (a.out_sum_w && lane == 0) a.out_sum_w[e] = S;
    if (!a.out_val) return;
    const double invS = 1.0 / S;
    const double invS2 = 1.0 / (S * S);
    const double g = t_g[idx * C + c];
    const double wg = w * g;
    double term = 0.0;
    if (STD) {
        const double dg = t_d[idx * C + c] * sdv;
        term = merge_var_term(w, dw, g, dg, invS, invS2, it);
    }
    double acc = 0.0, var = 0.0;
    for (int i = 0; i < N; ++i) {
        const double wgi = readlane_f64(wg, i), iti = readlane_f64(it, i);
        acc = (i == 0) ? wgi * iti : fma(wgi, iti, acc);
        if (STD) {
            const double ti = readlane_f64(term, i);
            var = (i == 0) ? ti * ti : fma(ti, ti, var);
        }
    }
    double val = acc / S;
    double sd = STD ? sqrt(var) : 0.0;
    if (a.has_flat) flat_field_apply(a, e, c, STD, val, sd);
    if (lane == 0) {
        store_out<OUT>(a.out_val, e, val);
        if (STD) store_out<OUT>(a.out_std, e, sd);
    }
}

// (scan_chunk_hotbits, lane_hotmask and the scan itself: hm_merge_hot_scan.h)
// (the hot-element queue's layout in the caller's workspace: hm_merge_dev.h)

// merge_fixup_hot: every lane scans 16 consecutive elements of every distinct dark map; elements with at least one hot
// frame are recomputed, one at a time, by the wave. This is the path WITHOUT a workspace: one element per wave at a time
// makes it collapse on dense maps (15 us of one wave per hot element) - callers that can pass a workspace should.
template <bool F64IN, bool STD, int OUT = OUT_F64, bool LUT = false, typename SD = double>
__global__ __launch_bounds__(256) void merge_fixup_hot(const MergeK a) {
    __shared__ double t_w[256], t_dw[256], t_g[256 * HM_MAX_CHANNELS], t_d[256 * HM_MAX_CHANNELS];
    fill_plain_tables<F64IN, STD>(a, t_w, t_dw, t_g, t_d);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t n_chunks = (a.n_elems + 15) / 16;
    const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
    // chunks are dealt 64 at a time to a wave, so the trip count is wave-uniform
    for (int64_t cb = wave0 * 64; cb < n_chunks; cb += n_waves * 64) {
        const int64_t chunk = cb + lane;
        const int64_t e0 = a.elem0 + chunk * 16;                            // relative to row0
        uint32_t hotbits = 0;
        if (chunk < n_chunks) {
            const int64_t left = a.elem0 + a.n_elems - e0;
            hotbits = scan_chunk_hotbits<uint8_t>(a, 255u, e0, left < 16 ? static_cast<int>(left) : 16);
        }
        unsigned long long pending = __ballot(hotbits != 0);
        while (pending) {                                                    // rare
            const int src = __ffsll(static_cast<long long>(pending)) - 1;
            pending &= pending - 1;
            uint32_t bits = __builtin_amdgcn_readlane(hotbits, src);
            const int64_t base = a.elem0 + (cb + src) * 16;
            while (bits) {
                const int b = __ffs(static_cast<int>(bits)) - 1;
                bits &= bits - 1;
                fixup_element<F64IN, STD, OUT, LUT, SD>(a, t_w, t_dw, t_g, t_d, base + b);
            }
        }
    }
}

// merge_scan_hot (hm_merge_hot.hip; it reads no std): the scan alone, launched through launch_scan_hot() from every unit
int launch_scan_hot(const MergeK& k, uint32_t* ws, uint32_t capacity, hipStream_t st);

// ------------------------------------------------------------------------------------------------
// Per-LANE hot-pixel patch: every lane recomputes its own hot element, so up to 64 elements are in flight per wave and their
// memory round trips overlap. patch_element_k3() is merge_one_element()'s operation sequence written so that the dependent
// rounds are few: the dark bytes of 8 frames at a time, then - for kPatchFB frames at a time - ALL nine neighbours of every frame
// with select-ed addresses (a frame that is not hot reads its own element nine times: no branch sits between the loads and
// the compiler's wait counts stay exact), the 19-exchange median network, and the frames' arithmetic in frame order.
// Pass 1 leaves every frame's (filtered) value in a per-thread LDS column for pass 2; the std medians are taken in pass 2.
// Other kernel sizes (5, 7) and float64 stacks of more than kPatchF64Frames frames go through merge_one_element<HOT_LANE>.
// ------------------------------------------------------------------------------------------------
#ifndef HM_PATCH_HOT_ONLY
#define HM_PATCH_HOT_ONLY 1             // 1: neighbour loads only in the lanes (and waves) where the frame is hot; 0: select-ed addresses, no branch
#endif
constexpr int kPatchFB = 4;             // frames whose nine neighbour loads are issued together (float64 values / stds)
constexpr int kPatchFBU8 = 8;           // the same for uint8 values (one VGPR each)
constexpr int kPatchF64Frames = 16;     // float64 stacks: frames kept in LDS between the passes (8 B x 256 threads each)

template <bool F64IN, bool STD, int OUT = OUT_F64, bool LUT = false, typename SD = double>
__device__ __forceinline__ void patch_element_k3(const MergeK& a, const double* t_w, const double* t_dw, const double* t_g, const double* t_d,
                                                 std::conditional_t<F64IN, double, uint8_t>* keep /* LDS, this thread's column, stride 256 */,
                                                 int64_t e, uint32_t hotmask) {
    using T = std::conditional_t<F64IN, double, uint8_t>;
    using V = typename MedianKey<T>::type;
    const int C = a.C, N = a.n_frames;
    const int64_t ei = a.in_off + e;
    const int c = static_cast<int>(e % C);
    int64_t row, col; int cc;
    elem_to_pixel(a, e, row, col, cc);
    const int64_t wc = a.W * C;
    const int64_t dy[3] = {(reflect_index(row - 1, a.H) - row) * wc, 0, (reflect_index(row + 1, a.H) - row) * wc};
    const int64_t dx[3] = {(reflect_index(col - 1, a.W) - col) * C, 0, (reflect_index(col + 1, a.W) - col) * C};
    // ---- pass 1: filtered values, S = sum_i w_i (exposure_series.py:340)
    constexpr int FBV = F64IN ? kPatchFB : kPatchFBU8;
    double S = 0.0;
    for (int i0 = 0; i0 < N; i0 += FBV) {
        V p[FBV][9];
#pragma unroll
        for (int f = 0; f < FBV; ++f) {
            if (i0 + f < N) {
                const T* fr = static_cast<const T*>(a.frame[i0 + f]) + ei;
                const bool hot = (hotmask >> (i0 + f)) & 1u;
#if HM_PATCH_HOT_ONLY
                // the frame's own element for every lane; its eight neighbours only in the lanes where THIS frame is hot (a wave in
                // which it is hot nowhere skips them): with one map per frame an element is typically hot in one frame of N
                const V centre = static_cast<V>(fr[0]);
#pragma unroll
                for (int q = 0; q < 9; ++q) p[f][q] = centre;
                if (hot) {
#pragma unroll
                    for (int q = 0; q < 9; ++q)
                        if (q != 4) p[f][q] = static_cast<V>(fr[dy[q / 3] + dx[q % 3]]);
                }
#else
#pragma unroll
                for (int q = 0; q < 9; ++q) p[f][q] = static_cast<V>(fr[hot ? dy[q / 3] + dx[q % 3] : int64_t{0}]);
#endif
            }
        }
#pragma unroll
        for (int f = 0; f < FBV; ++f) {
            if (i0 + f < N) {
                const V v = median9<T>(p[f]);
                keep[(i0 + f) * 256] = static_cast<T>(v);
                double w;
                if constexpr (F64IN) w = gauss_weight(v - 0.5);                          // measurand.py:615
                else w = t_w[v];
                S = (i0 + f == 0) ? w : S + w;
            }
        }
    }
    if (a.out_sum_w) a.out_sum_w[e] = S;
    if (!a.out_val) return;
    const double invS = 1.0 / S;
    const double invS2 = 1.0 / (S * S);                                                  // 1 / S**2, exposure_series.py:343
    // ---- pass 2: exposure_series.py:382-389
    double acc = 0.0, var = 0.0;
    for (int i0 = 0; i0 < N; i0 += kPatchFB) {
        double sp[STD ? kPatchFB : 1][9];
        if constexpr (STD) {
#pragma unroll
            for (int f = 0; f < kPatchFB; ++f) {
                if (i0 + f < N) {
                    // the std of element ei + off: the frame's std image, or (LUT) the per-DN table entry of the frame's value there - the
                    // UNFILTERED value: the median is taken over the mapped neighbourhood
                    const SD* sr = LUT ? nullptr : a.template sd_as<SD>(i0 + f) + ei;
                    const StdLutAt<T> lut_at{static_cast<const T*>(a.frame[i0 + f]) + ei, a.std_lut, C, c};
                    auto std_at = [&](int64_t off) -> double { if constexpr (LUT) return lut_at(off); else return static_cast<double>(sr[off]); };
                    const bool hot = (hotmask >> (i0 + f)) & 1u;
#if HM_PATCH_HOT_ONLY
                    const double centre = std_at(0);
#pragma unroll
                    for (int q = 0; q < 9; ++q) sp[f][q] = centre;
                    if (hot) {
#pragma unroll
                        for (int q = 0; q < 9; ++q)
                            if (q != 4) sp[f][q] = std_at(dy[q / 3] + dx[q % 3]);
                    }
#else
#pragma unroll
                    for (int q = 0; q < 9; ++q) sp[f][q] = std_at(hot ? dy[q / 3] + dx[q % 3] : int64_t{0});
#endif
                }
            }
        }
#pragma unroll
        for (int f = 0; f < kPatchFB; ++f) {
            if (i0 + f < N) {
                const int i = i0 + f;
                double w, dw;
                uint32_t idx;
                if constexpr (F64IN) {
                    const double v = keep[i * 256];
                    const double dv = v - 0.5;
                    w = gauss_weight(dv);
                    dw = gauss_dweight(dv, w);                                               // measurand.py:616
                    idx = lut_index(v);   // measurand.py:503
                } else {
                    idx = keep[i * 256];
                    w = t_w[idx];
                    dw = STD ? t_dw[idx] : 0.0;
                }
                const double g = t_g[idx * C + c];
                const double it = a.inv_t[i];
                const double wg = w * g;
                acc = (i == 0) ? wg * it : fma(wg, it, acc);                             // :388 numerator
                if constexpr (STD) {
                    const double sv = median9<double>(sp[f]);
                    const double dg = t_d[idx * C + c] * sv;                             // measurand.py:512
                    const double term = merge_var_term(w, dw, g, dg, invS, invS2, it);   // :389
                    var = (i == 0) ? term * term : fma(term, term, var);
                }
            }
        }
    }
    double val = acc / S;
    double sd = STD ? sqrt(var) : 0.0;                                                   // :394
    if (a.has_flat) flat_field_apply(a, e, c, STD, val, sd);
    store_out<OUT>(a.out_val, e, val);
    if (STD) store_out<OUT>(a.out_std, e, sd);
}

template <bool F64IN, bool STD, int OUT = OUT_F64, bool LUT = false, typename SD = double>
__device__ __forceinline__ void patch_element(const MergeK& a, const double* t_w, const double* t_dw, const double* t_g, const double* t_d,
                                              char* keep_lds, int64_t e, uint32_t hotmask) {
    using T = std::conditional_t<F64IN, double, uint8_t>;
    if (a.median_k == 3 && (!F64IN || a.n_frames <= kPatchF64Frames))                    // wave-uniform
        patch_element_k3<F64IN, STD, OUT, LUT, SD>(a, t_w, t_dw, t_g, t_d, reinterpret_cast<T*>(keep_lds) + threadIdx.x, e, hotmask);
    else
        merge_one_element<F64IN, STD, HOT_LANE, OUT, LUT, SD>(a, t_w, t_dw, t_g, t_d, e, true);
}
inline int patch_keep_bytes(bool f64in, int n_frames, int median_k) {
    if (median_k != 3 || (f64in && n_frames > kPatchF64Frames)) return 16;
    return n_frames * 256 * (f64in ? 8 : 1);
}

// merge_patch_hot: the queue's elements, one per lane. The grid is fixed (the host does not know the count), so the entries are
// dealt to ALL its waves in blocks of B = ceil(count / waves) <= 64 consecutive entries: a short queue is spread over the
// whole chip (one or a few active lanes per wave: the latency of one element, not of 64), a long one fills the waves (and
// consecutive lanes take consecutive entries, which a wave's span put there in element order, so neighbouring lanes touch
// neighbouring cache lines). Workgroups beyond the queue leave before they build their tables.
// If the scan raised the overflow flag (more hot elements than the workspace holds: a quarter of the image with the recommended
// size) the queue is ignored: every lane looks at its own elements' dark bytes and patches the hot ones.
template <bool F64IN, bool STD, int OUT = OUT_F64, bool LUT = false, typename SD = double>
__global__ __launch_bounds__(256) void merge_patch_hot(const MergeK a, const uint32_t* ws, uint32_t bmax) {
    __shared__ double t_w[256], t_dw[256], t_g[256 * HM_MAX_CHANNELS], t_d[256 * HM_MAX_CHANNELS];
    extern __shared__ __attribute__((aligned(16))) char keep_lds[];
    const uint32_t count = __builtin_amdgcn_readfirstlane(ws[0]);
    const uint32_t overflow = __builtin_amdgcn_readfirstlane(ws[1]);
    const uint32_t n_waves = gridDim.x * 4u;
    uint32_t B = (count + n_waves - 1u) / n_waves;
    B = B > bmax ? bmax : B;
    if (overflow == 0u && count == 0u) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    // Blocks of B consecutive entries - consecutive in IMAGE order: the pieces are walked through the scan's piece table - are dealt
    // iteration by iteration: in iteration `it` the logical workgroup l takes blocks (it * G + l) * 4 + wave, and workgroups that run on
    // the same XCD (blockIdx % 8: round-robin dispatch) are neighbours in l. At any moment one XCD works on ONE run of image rows, and
    // the lines its hot elements share (rows r - 1, r, r + 1 of every frame) are requested from one L2 at about the same time: at a
    // density of 5e-2 a workgroup that owned a contiguous part of the queue over all its iterations fetched every line 2.3 times
    // (profiles/r03e_hot5e2_patch_rocprof_summary.md; 2 270 -> 1 820 us per merge with the interleaved order, r03m_ab_patch_order.log).
    // HM_PATCH_ORDER 1 = that first mapping.
#ifndef HM_PATCH_ORDER
#define HM_PATCH_ORDER 0
#endif
    const uint32_t* const table = ws + kHotQueueHeader;
    const uint32_t* const queue = table + 2u * hot_piece_slots(a.n_elems);
    const uint32_t iters = B ? (count + n_waves * B - 1u) / (n_waves * B) : 0u;
    const uint32_t per_xcd = (gridDim.x + 7u) / 8u;
    const uint32_t logical = gridDim.x % 8u == 0u ? (blockIdx.x % 8u) * per_xcd + blockIdx.x / 8u : blockIdx.x;
    auto entry_of = [&](uint32_t it) -> uint64_t {
        if (HM_PATCH_ORDER == 1) return static_cast<uint64_t>(logical) * 4u * B * iters + (static_cast<uint64_t>(it) * 4u + wave) * B + lane;
        return ((static_cast<uint64_t>(it) * gridDim.x + logical) * 4u + wave) * B + lane;
    };
    if (overflow == 0u && static_cast<uint64_t>(logical) * 4u * B * (HM_PATCH_ORDER == 1 ? iters : 1u) >= count) return;
    // image-order position -> queue slot: exclusive prefix of the piece counts in LDS (one piece = 8 bytes of table per 65 536 elements)
    __shared__ uint32_t s_pref[kHotPiecesLds + 1], s_off[kHotPiecesLds], s_wsum[4];
    const uint32_t n_pieces = __builtin_amdgcn_readfirstlane(ws[2]);
    const bool ordered = overflow == 0u && n_pieces <= static_cast<uint32_t>(kHotPiecesLds) && HM_PATCH_ORDER == 0;
    if (ordered) {
        constexpr uint32_t PER = kHotPiecesLds / 256;
        uint32_t cnt[PER], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
            const uint32_t pc = threadIdx.x * PER + k;
            cnt[k] = pc < n_pieces ? table[2u * pc + 1u] : 0u;
            if (pc < n_pieces) s_off[pc] = table[2u * pc];
            sum += cnt[k];
        }
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= static_cast<uint32_t>(d)) incl += up;
        }
        if (lane == 63u) s_wsum[wave] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (uint32_t w = 0; w < wave; ++w) run += s_wsum[w];
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
            const uint32_t pc = threadIdx.x * PER + k;
            if (pc <= n_pieces) s_pref[pc] = run;
            run += cnt[k];
        }
        if (threadIdx.x == 255) s_pref[kHotPiecesLds] = run;
        __syncthreads();
    }
    auto slot_of = [&](uint64_t pos) -> uint64_t {                  // pos < count
        if (!ordered) return pos;
        uint32_t lo = 0, hi = n_pieces;                               // the piece p with s_pref[p] <= pos < s_pref[p + 1]
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_pref[mid] <= static_cast<uint32_t>(pos)) lo = mid; else hi = mid;
        }
        return static_cast<uint64_t>(s_off[lo]) + (static_cast<uint32_t>(pos) - s_pref[lo]);
    };
    // the first entry and its dark bytes are fetched while the workgroup builds its tables (a short queue is one entry per lane:
    // its latency is the kernel's duration)
    int64_t e_first = 0;
    uint32_t hot_first = 0;
    if (overflow == 0u && lane < B && entry_of(0) < count) {
        e_first = static_cast<int64_t>(queue[slot_of(entry_of(0))]);
        hot_first = lane_hotmask<uint8_t>(a, a.in_off + e_first, 255u);
    }
    fill_plain_tables<F64IN, STD>(a, t_w, t_dw, t_g, t_d);
    __syncthreads();
    if (overflow != 0u) {
        const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
        for (int64_t q = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; q < a.n_elems; q += stride) {
            const int64_t e = a.elem0 + q;
            const uint32_t hotmask = lane_hotmask<uint8_t>(a, a.in_off + e, 255u);
            if (hotmask) patch_element<F64IN, STD, OUT, LUT, SD>(a, t_w, t_dw, t_g, t_d, keep_lds, e, hotmask);
        }
        return;
    }
    for (uint32_t it = 0; it < iters; ++it) {
        const uint64_t q = entry_of(it);
        if (lane < B && q < count) {
            int64_t e = e_first;
            uint32_t hotmask = hot_first;
            if (it != 0u) {
                e = static_cast<int64_t>(queue[slot_of(q)]);
                hotmask = lane_hotmask<uint8_t>(a, a.in_off + e, 255u);
            }
            patch_element<F64IN, STD, OUT, LUT, SD>(a, t_w, t_dw, t_g, t_d, keep_lds, e, hotmask);
        }
    }
}

// The one place that names the instantiations of this header's three kernel templates. A family wraps one of them (all of its instantiations
// share a function type); pick_kernel() maps a call to its instantiation, or to nullptr for what no unit holds: SD = float
// (hm_merge_std_f32) has std calls only, without the per-DN table (the dispatcher sends nothing else; the launchers answer HM_EINVAL).
#define HM_HOT_FAMILY(K, ...) \
    struct K##_family { \
        using fn_t = void (*)(__VA_ARGS__); \
        template <bool F, bool S, int OUT, bool LUT, typename SD> static fn_t get() { return &K<F, S, OUT, LUT, SD>; } \
    };
HM_HOT_FAMILY(merge_generic, const MergeK)
HM_HOT_FAMILY(merge_fixup_hot, const MergeK)
HM_HOT_FAMILY(merge_patch_hot, const MergeK, const uint32_t*, uint32_t)
#undef HM_HOT_FAMILY
template <typename FAMILY, int OUT, typename SD>
typename FAMILY::fn_t pick_kernel(const MergeK& k, bool f64in, bool with_std) {
    const bool lut = with_std && k.std_lut;
    if constexpr (std::is_same_v<SD, float>) {
        if (!with_std || lut) return nullptr;
        return f64in ? FAMILY::template get<true, true, OUT, false, float>() : FAMILY::template get<false, true, OUT, false, float>();
    } else {
        if (lut) return f64in ? FAMILY::template get<true, true, OUT, true, double>() : FAMILY::template get<false, true, OUT, true, double>();
        if (f64in) return with_std ? FAMILY::template get<true, true, OUT, false, double>() : FAMILY::template get<true, false, OUT, false, double>();
        return with_std ? FAMILY::template get<false, true, OUT, false, double>() : FAMILY::template get<false, false, OUT, false, double>();
    }
}

template <int OUT, typename SD>
int launch_generic(const MergeK& k, bool f64in, bool with_std, hipStream_t st) {
    const unsigned grid = stream_grid(k.n_elems, 256, 8);
    if (describe_only("merge_generic<f64in=%d,std=%d>", f64in, with_std)) return HM_OK;
    const auto fn = pick_kernel<merge_generic_family, OUT, SD>(k, f64in, with_std);
    if (!fn) return HM_EINVAL;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(256), 0, st, k);
    return launch_status();
}

template <int OUT, typename SD>
int launch_fixup(const MergeK& k, bool f64in, bool with_std, hipStream_t st) {
    const int64_t chunks = (k.n_elems + 15) / 16;
    const unsigned grid = stream_grid(chunks, 256, 8);
    if (describe_only("merge_fixup_hot<f64in=%d,std=%d>", f64in, with_std)) return HM_OK;
    const auto fn = pick_kernel<merge_fixup_hot_family, OUT, SD>(k, f64in, with_std);
    if (!fn) return HM_EINVAL;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(256), 0, st, k);
    return launch_status();
}

// the queue path of the hot-pixel pass: zero the counters, scan the dark maps into the queue, patch the queued elements;
// on overflow merge_patch_hot goes over the whole tile instead of the queue (a queue that was too small costs time, never correctness)
template <int OUT, typename SD>
int launch_hot_queue(const MergeK& k, bool f64in, bool with_std, uint32_t* ws, size_t ws_bytes, hipStream_t st) {
    const size_t head = static_cast<size_t>(kHotQueueHeader) + 2u * hot_piece_slots(k.n_elems);     // counters + piece table, in words
    const size_t words = ws_bytes / 4 - head;
    const uint32_t capacity = static_cast<uint32_t>(words > 0xffffffffull ? 0xffffffffull : words);
    if (describe_only("merge_scan_hot")) {
        describe_only("merge_patch_hot<f64in=%d,std=%d>", f64in, with_std);
        return HM_OK;
    }
    // (the counters were zeroed by the streaming kernel of this call - MergeK::hot_reset; the scan writes every table entry it owns)
    int rc = launch_scan_hot(k, ws, capacity, st);
    if (rc != HM_OK) return rc;
    // The grid is what the chip holds AT ONCE (the kernel's occupancy: 3-6 workgroups per CU, by registers): every workgroup is then
    // resident from the start and a sparse queue costs the latency of one element. A grid of 8 per CU ran its workgroups in three
    // rounds at 3 resident per CU - 57-65 us for 35 000 queued elements, each round the same dependent chain of memory round trips.
    const int keep = patch_keep_bytes(f64in, k.n_frames, k.median_k);
    const auto kernel = pick_kernel<merge_patch_hot_family, OUT, SD>(k, f64in, with_std);
    if (!kernel) return HM_EINVAL;
    const void* fn = reinterpret_cast<const void*>(kernel);
    // (the query costs a few microseconds of host time: remembered per kernel, LDS size and device, under a mutex - hm_merge may be called
    // from several host threads)
    static struct { const void* fn; int keep, dev, per_cu; } seen[16];
    static int n_seen = 0;
    static std::mutex seen_lock;
    int per_cu = 0, dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> hold(seen_lock);
        for (int i = 0; i < n_seen; ++i)
            if (seen[i].fn == fn && seen[i].keep == keep && seen[i].dev == dev) per_cu = seen[i].per_cu;
    }
    if (per_cu == 0) {
        // (gfx950 has 160 KB of LDS per workgroup; the kernel's 36 KB of tables + up to 32 KB of kept float64 frames fit. Should a device
        // report that not even one workgroup fits, -1 is remembered and the workspace-free pass runs instead - never a failing launch.)
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, static_cast<size_t>(keep)) != hipSuccess) { (void)hipGetLastError(); per_cu = 2; }
        if (per_cu < 1) per_cu = -1;
        if (per_cu > 8) per_cu = 8;
        std::lock_guard<std::mutex> hold(seen_lock);
        if (n_seen < 16) { seen[n_seen].fn = fn; seen[n_seen].keep = keep; seen[n_seen].dev = dev; seen[n_seen].per_cu = per_cu; ++n_seen; }
    }
    if (per_cu < 0) return launch_fixup<OUT, SD>(k, f64in, with_std, st);
    if (const int e = tune_env("HM_TUNE_PATCH_WG_PER_CU", 1, 16)) per_cu = e;
    const unsigned grid = stream_grid(k.n_elems, 256, per_cu);
    uint32_t bmax = 64;
    if (const int e = tune_env("HM_TUNE_PATCH_BMAX", 1, 64)) bmax = static_cast<uint32_t>(e);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), keep, st, k, static_cast<const uint32_t*>(ws), bmax);
    return launch_status();
}

}  // namespace hm
