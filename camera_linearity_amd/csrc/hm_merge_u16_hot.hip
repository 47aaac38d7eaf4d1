// hm_merge_u16_hot.hip - the hot-pixel pass of the uint16 merge (hm_merge_u16_darks; gfx950): uint16 dark maps, frame i hot at an element
// iff (dark DN & M) >= dark_min_dn[i], M = 2^bit_depth - 1. It runs stream-ordered after hm_merge_u16's kernels, which never read a dark
// map, and recomputes the elements that have a hot frame with the k x k medians of the masked DNs (and of the stds) substituted.
//
//   merge_u16_scan_hot    merge_scan_hot for 2-byte maps: every distinct (map, threshold) read once, hot elements compacted into the
//                         queue of hm_merge_dev.h (header words, piece table in image order, queue), one atomic add per workgroup and round.
//   merge_u16_patch_hot   one queued element per lane: merge_u16_element's operation sequence with the medians substituted, every table
//                         gathered from global memory at idx = DN & M (no table in LDS at any depth; LDS holds only the lane's filtered DNs
//                         between the two passes). The queue is dealt as it lies, in blocks of B = ceil(count / waves) <= 64 consecutive
//                         entries per wave (no image-ordered walk through the piece table). With the scan's overflow flag raised, or without
//                         a workspace (queue=0), every lane tests its own elements' dark DNs and patches the hot ones.
#include "hm_merge_u16.h"

namespace hm {

constexpr int kU16ScanRound = 4;        // chunks of 16 elements (two 16-byte loads) a lane scans per round: 65 536 elements per workgroup and round
constexpr int kU16ScanBlock = 1024;
constexpr int kU16PatchBlock = 256;

// distinct (map, threshold) pairs: bit i set = frame i's map is read (wave-uniform)
__device__ __forceinline__ uint32_t distinct_darks(const MergeK& a) {
    uint32_t distinct = 0;
    for (int i = 0; i < a.n_frames; ++i) {
        const uint8_t* d = a.dark[i];
        if (!d) continue;
        bool seen = false;                                          // same map + threshold as an earlier frame
        for (int k = 0; k < i; ++k) seen = seen || (a.dark[k] == d && a.dark_min[k] == a.dark_min[i]);
        if (!seen) distinct |= 1u << i;
    }
    return distinct;
}

// hot bits of a chunk of cnt <= 16 elements starting at e0 (relative to row0), one 2-byte load per element and map: maps that are not
// 16-byte aligned at the tile's first element, and the tile's last, partial chunk
__device__ __forceinline__ uint32_t scan_chunk_hotbits16(const MergeK& a, uint32_t distinct, uint32_t mask, int64_t e0, int cnt) {
    uint32_t hotbits = 0;
    for (uint32_t left = distinct; left; left &= left - 1) {        // wave-uniform loop over the distinct maps
        const int i = __builtin_amdgcn_readfirstlane(__ffs(static_cast<int>(left)) - 1);
        const uint16_t* p = dark16(a, i) + a.in_off + e0;
        const uint32_t thr = static_cast<uint32_t>(a.dark_min[i]);
        for (int b = 0; b < cnt; ++b) hotbits |= ((static_cast<uint32_t>(p[b]) & mask) >= thr) ? (1u << b) : 0u;
    }
    return hotbits;
}

// merge_scan_hot's decomposition (hm_merge_hot.hip) with 2-byte dark DNs: a lane's chunk is 16 consecutive elements = two 16-byte loads,
// a wave's span 1024 elements, a workgroup's round 65 536: the queue layout, its piece table and the workspace sizes are the 8-bit pass's.
__global__ __launch_bounds__(kU16ScanBlock) void merge_u16_scan_hot(const MergeK a, const uint32_t mask, uint32_t* ws, uint32_t capacity) {
    uint32_t* const table = ws + kHotQueueHeader;
    uint32_t* const queue = table + 2u * hot_piece_slots(a.n_elems);
    __shared__ uint32_t s_tot[kU16ScanBlock / 64];
    __shared__ uint32_t s_base, s_ok;
    constexpr uint32_t WPB = kU16ScanBlock / 64;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_chunks = (a.n_elems + 15) / 16;
    const int64_t n_spans = (n_chunks + 63) / 64;
    const int64_t n_waves = static_cast<int64_t>(gridDim.x) * WPB;
    const int64_t wave_global = static_cast<int64_t>(blockIdx.x) * WPB + wave;
    const int64_t rounds = (n_spans + n_waves * kU16ScanRound - 1) / (n_waves * kU16ScanRound);
    // `wide` = every map that is read can be read with aligned 16-byte loads (map + in_off 16-byte aligned: elem0 and the chunk starts
    // are multiples of 16 elements)
    const uint32_t distinct = distinct_darks(a);
    bool wide = (a.elem0 & 15) == 0;
    for (uint32_t left = distinct; left; left &= left - 1) {
        const int i = __builtin_amdgcn_readfirstlane(__ffs(static_cast<int>(left)) - 1);
        wide = wide && (reinterpret_cast<uintptr_t>(dark16(a, i) + a.in_off) & 15) == 0;
    }
    const int64_t n_full = a.n_elems / 16;                                  // whole 16-element chunks; a last partial one goes the slow way
    for (int64_t r = 0; r < rounds; ++r) {
        uint32_t hb[kU16ScanRound];
        uint32_t mine = 0;
        if (wide) {
            // no load sits behind a lane-dependent branch: the round's loads of a map are issued back to back (a chunk past the end
            // re-reads chunk 0 and is masked afterwards), then compared
            int64_t off[kU16ScanRound];
            bool valid[kU16ScanRound];
#pragma unroll
            for (int k = 0; k < kU16ScanRound; ++k) {
                const int64_t chunk = (((r * n_waves + wave_global) * kU16ScanRound) + k) * 64 + lane;
                valid[k] = chunk < n_full;
                off[k] = a.in_off + a.elem0 + (valid[k] ? chunk : 0) * 16;   // in elements; < in_off + elem0 + n_full * 16 <= the tile's end
                hb[k] = 0;
            }
            if (n_full > 0) {
                for (uint32_t left = distinct; left; left &= left - 1) {
                    const int i = __builtin_amdgcn_readfirstlane(__ffs(static_cast<int>(left)) - 1);
                    const uint16_t* d = dark16(a, i);
                    const uint32_t thr = static_cast<uint32_t>(a.dark_min[i]);
                    u32x4 v[kU16ScanRound][2];
#pragma unroll
                    for (int k = 0; k < kU16ScanRound; ++k) {
                        const u32x4* p = reinterpret_cast<const u32x4*>(d + off[k]);
                        v[k][0] = __builtin_nontemporal_load(p);
                        v[k][1] = __builtin_nontemporal_load(p + 1);
                    }
#pragma unroll
                    for (int k = 0; k < kU16ScanRound; ++k) {
                        const uint32_t w8[8] = {v[k][0].x, v[k][0].y, v[k][0].z, v[k][0].w, v[k][1].x, v[k][1].y, v[k][1].z, v[k][1].w};
#pragma unroll
                        for (int b = 0; b < 16; ++b) hb[k] |= (((w8[b >> 1] >> (16 * (b & 1))) & mask) >= thr) ? (1u << b) : 0u;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kU16ScanRound; ++k) {
                const int64_t chunk = (((r * n_waves + wave_global) * kU16ScanRound) + k) * 64 + lane;
                if (!valid[k]) hb[k] = 0;
                if (chunk == n_full && chunk < n_chunks)                    // the tile's last, partial chunk (one lane of one wave)
                    hb[k] = scan_chunk_hotbits16(a, distinct, mask, a.elem0 + chunk * 16, static_cast<int>(a.n_elems - chunk * 16));
                mine += static_cast<uint32_t>(__popc(hb[k]));
            }
        } else {
#pragma unroll
            for (int k = 0; k < kU16ScanRound; ++k) {
                const int64_t chunk = (((r * n_waves + wave_global) * kU16ScanRound) + k) * 64 + lane;
                hb[k] = 0;
                if (chunk < n_chunks) {
                    const int64_t left = a.n_elems - chunk * 16;
                    hb[k] = scan_chunk_hotbits16(a, distinct, mask, a.elem0 + chunk * 16, left < 16 ? static_cast<int>(left) : 16);
                }
                mine += static_cast<uint32_t>(__popc(hb[k]));
            }
        }
        uint32_t incl = mine;                                               // inclusive prefix sum over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= static_cast<uint32_t>(d)) incl += up;
        }
        if (lane == 63u) s_tot[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = 0;
#pragma unroll
            for (uint32_t w = 0; w < WPB; ++w) total += s_tot[w];
            uint32_t base = 0, ok = 1;
            if (total) {
                base = atomicAdd(&ws[0], total);
                if (base + total > capacity || base + total < base) {       // queue full: flag it, the patch kernel goes over the whole tile instead
                    atomicOr(&ws[1], 1u);
                    ok = 0;
                }
            }
            s_base = base; s_ok = ok;
            const uint32_t piece = static_cast<uint32_t>(r * gridDim.x + blockIdx.x);          // image order
            table[2u * piece] = ok ? base : 0u;
            table[2u * piece + 1u] = ok ? total : 0u;
            if (blockIdx.x == 0 && r == 0) ws[2] = static_cast<uint32_t>(rounds * gridDim.x);
        }
        __syncthreads();
        if (s_ok && mine) {
            uint32_t off = s_base + (incl - mine);
            for (uint32_t w = 0; w < wave; ++w) off += s_tot[w];
            uint32_t* q = queue + off;                                      // off + mine <= base + total <= capacity
#pragma unroll
            for (int k = 0; k < kU16ScanRound; ++k) {
                uint32_t bits = hb[k];
                const int64_t chunk = (((r * n_waves + wave_global) * kU16ScanRound) + k) * 64 + lane;
                const uint32_t first = static_cast<uint32_t>(a.elem0 + chunk * 16);   // < 2^32 (host check)
                while (bits) {
                    const int b = __ffs(static_cast<int>(bits)) - 1;
                    bits &= bits - 1;
                    *q++ = first + static_cast<uint32_t>(b);
                }
            }
        }
        __syncthreads();                                                    // s_tot / s_base are rewritten in the next round
    }
}

// frames that are hot at input element ei: bit i
__device__ __forceinline__ uint32_t lane_hotmask16(const MergeK& a, int64_t ei, uint32_t mask) {
    uint32_t hotmask = 0;
    const int N = a.n_frames;
    for (int i0 = 0; i0 < N; i0 += 8) {
        uint32_t d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            d[k] = 0;
            if (i0 + k < N && a.dark[i0 + k]) d[k] = dark16(a, i0 + k)[ei];                  // wave-uniform condition
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (i0 + k < N && a.dark[i0 + k]) hotmask |= (static_cast<int>(d[k] & mask) >= a.dark_min[i0 + k]) ? (1u << (i0 + k)) : 0u;
    }
    return hotmask;
}

// element accessors of the k x k medians: index = (buffer row * W + column) * C + c (lane_median_of, hm_common.h)
struct DnAt {
    const uint16_t* f; uint32_t mask;
    __device__ __forceinline__ uint32_t operator()(int64_t i) const { return static_cast<uint32_t>(f[i]) & mask; }
};

// merge_u16_element (hm_merge_u16.hip) with the medians of the hot frames substituted: the masked DN of a hot frame is the k x k median
// of the masked DNs around it, its std the k x k median of the std neighbourhood. The neighbourhood is read only where the frame is hot.
// keep: this thread's LDS column (stride kU16PatchBlock) for the filtered DNs between the two passes.
template <bool STD, int OUT>
__device__ __forceinline__ void patch_u16_element(const MergeK& a, uint32_t mask, uint16_t* keep, int64_t e, uint32_t hotmask) {
    const int C = a.C, N = a.n_frames, k = a.median_k;
    const int64_t ei = a.in_off + e;
    int64_t row, col; int c;
    elem_to_pixel(a, e, row, col, c);
    double S = 0.0;
    for (int i = 0; i < N; ++i) {
        const uint16_t* f = static_cast<const uint16_t*>(a.frame[i]);
        uint32_t idx = static_cast<uint32_t>(f[ei]) & mask;
        if ((hotmask >> i) & 1u) idx = lane_median_of<uint16_t>(DnAt{f, mask}, a.H, a.W, C, a.buf_row0, row, col, c, k);
        keep[i * kU16PatchBlock] = static_cast<uint16_t>(idx);
        const double w = a.w_lut[idx];
        S = (i == 0) ? w : S + w;                                       // exposure_series.py:340
    }
    if (a.out_sum_w) a.out_sum_w[e] = S;
    if (!a.out_val) return;
    const double invS = 1.0 / S;
    const double invS2 = 1.0 / (S * S);                                 // 1 / S**2, exposure_series.py:343
    double acc = 0.0, var = 0.0;
    for (int i = 0; i < N; ++i) {
        const uint32_t idx = keep[i * kU16PatchBlock];
        const double w = a.w_lut[idx];
        const double dw = STD ? a.dw_lut[idx] : 0.0;
        const double g = a.icrf[idx * C + c];
        const double it = a.inv_t[i];
        const double wg = w * g;
        acc = (i == 0) ? wg * it : fma(wg, it, acc);                    // :388 numerator
        if (STD) {
            double s = a.sd[i][ei];
            if ((hotmask >> i) & 1u) s = lane_median_of<double>(StdAt<double>{a.sd[i]}, a.H, a.W, C, a.buf_row0, row, col, c, k);
            const double dg = a.icrf_diff[idx * C + c] * s;             // measurand.py:512
            const double A = (dw * g + w * dg) * invS - ((dw * w) * g) * invS2;   // :389
            const double term = (A * dg) * it;
            var = (i == 0) ? term * term : fma(term, term, var);
        }
    }
    double val = acc / S;
    double sd = STD ? sqrt(var) : 0.0;                                  // :394
    if (a.has_flat) flat_field_apply(a, e, c, STD, val, sd);            // (the float64 flat field)
    store_out<OUT>(a.out_val, e, val);
    if (STD) store_out<OUT>(a.out_std, e, sd);
}

// ws == NULL: no queue (queue=0)
template <bool STD, int OUT>
__global__ __launch_bounds__(kU16PatchBlock) void merge_u16_patch_hot(const MergeK a, const uint32_t mask, const uint32_t* ws) {
    __shared__ uint16_t s_keep[HM_MAX_FRAMES * kU16PatchBlock];
    uint16_t* const keep = s_keep + threadIdx.x;
    uint32_t count = 0, overflow = 1;
    if (ws) {
        count = __builtin_amdgcn_readfirstlane(ws[0]);
        overflow = __builtin_amdgcn_readfirstlane(ws[1]);
    }
    if (overflow != 0u) {                                               // every lane tests its own elements
        const int64_t stride = static_cast<int64_t>(gridDim.x) * kU16PatchBlock;
        for (int64_t q = static_cast<int64_t>(blockIdx.x) * kU16PatchBlock + threadIdx.x; q < a.n_elems; q += stride) {
            const int64_t e = a.elem0 + q;
            const uint32_t hotmask = lane_hotmask16(a, a.in_off + e, mask);
            if (hotmask) patch_u16_element<STD, OUT>(a, mask, keep, e, hotmask);
        }
        return;
    }
    if (count == 0u) return;
    constexpr uint32_t WPB = kU16PatchBlock / 64;
    const uint32_t* const queue = ws + kHotQueueHeader + 2u * hot_piece_slots(a.n_elems);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * WPB;
    const uint64_t wave_global = static_cast<uint64_t>(blockIdx.x) * WPB + (threadIdx.x >> 6);
    uint64_t B = (count + n_waves - 1u) / n_waves;                      // a short queue is spread over all waves, a long one fills them
    B = B > 64u ? 64u : B;
    for (uint64_t base = wave_global * B; base < count; base += n_waves * B) {
        const uint64_t q = base + lane;
        if (lane < B && q < count) {                                    // count <= the queue's capacity (no overflow)
            const int64_t e = static_cast<int64_t>(queue[q]);          // < n_elems: the scan queues elements of the tile only
            patch_u16_element<STD, OUT>(a, mask, keep, e, lane_hotmask16(a, a.in_off + e, mask));
        }
    }
}

int launch_u16_hot(const MergeK& k, int bits, bool with_std, bool f32out, uint32_t* ws, size_t ws_bytes, hipStream_t st) {
    const uint32_t mask = (1u << bits) - 1u;
    if (ws) {
        if (!describe_only("merge_u16_scan_hot")) {
            const size_t head = static_cast<size_t>(kHotQueueHeader) + 2u * hot_piece_slots(k.n_elems);     // counters + piece table, in words
            const size_t words = ws_bytes / 4 - head;                                                       // >= 1 (the caller's size check)
            const uint32_t capacity = static_cast<uint32_t>(words > 0xffffffffull ? 0xffffffffull : words);
            // (the counters were zeroed by the first kernel of this call - MergeK::hot_reset; the scan writes every table entry it owns)
            const int64_t chunks = (k.n_elems + 15) / 16;
            hipLaunchKernelGGL(merge_u16_scan_hot, dim3(stream_grid(chunks, kU16ScanBlock, 1)), dim3(kU16ScanBlock), 0, st, k, mask, ws, capacity);
            const int rc = launch_status();
            if (rc != HM_OK) return rc;
        }
    }
    if (describe_only(ws ? "merge_u16_patch_hot<bits=%d,std=%d,k=%d>" : "merge_u16_patch_hot<bits=%d,std=%d,k=%d,queue=0>", bits, with_std, k.median_k))
        return HM_OK;
    const unsigned grid = stream_grid(k.n_elems, kU16PatchBlock, ws ? 4 : 8);
    const uint32_t* cws = ws;
#define HM_U16_PATCH(S, O) hipLaunchKernelGGL((merge_u16_patch_hot<S, O>), dim3(grid), dim3(kU16PatchBlock), 0, st, k, mask, cws)
    if (f32out) { if (with_std) HM_U16_PATCH(true, OUT_F32); else HM_U16_PATCH(false, OUT_F32); }
    else { if (with_std) HM_U16_PATCH(true, OUT_F64); else HM_U16_PATCH(false, OUT_F64); }
#undef HM_U16_PATCH
    return launch_status();
}

}  // namespace hm
