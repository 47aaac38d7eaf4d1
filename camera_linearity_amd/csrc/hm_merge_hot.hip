// hm_merge_hot.hip - the one-element-per-thread kernel and the hot-pixel pass of hm_merge_hot.h for float64 std frames (with their val-only
// and per-DN-table forms), and merge_scan_hot, which every form of the pass shares.
#include "hm_merge_hot.h"

namespace hm {

// merge_scan_hot: the scan alone. A wave scans kScanRound consecutive spans of 1024 elements per round (16 bytes per lane, map and
// span, the round's loads of a map issued together), a workgroup's 16 waves 64 consecutive spans = 65 536 elements (a few image
// rows: what lands next to each other in the queue shares its neighbour rows, which the patch kernel then finds in the cache).
// The waves add up their counts through LDS and ONE atomic add per workgroup
// and round reserves its piece of the queue (an atomic per wave and span serialised on the counter: 49 000 returning atomics on
// one address took 365 us at a density of 1e-3, profiles/r03c_hot_trace.txt). Every wave runs the same number of rounds (barriers).
// The order of the pieces in the queue depends on the order of the atomics; the patched image does not (every queued element is
// recomputed independently).
constexpr int kScanRound = 4;
constexpr int kScanBlock = 1024;
__global__ __launch_bounds__(kScanBlock) void merge_scan_hot(const MergeK a, uint32_t* ws, uint32_t capacity) {
    uint32_t* const table = ws + kHotQueueHeader;
    uint32_t* const queue = table + 2u * hot_piece_slots(a.n_elems);
    __shared__ uint32_t s_tot[kScanBlock / 64];
    __shared__ uint32_t s_base, s_ok;
    constexpr uint32_t WPB = kScanBlock / 64;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n_chunks = (a.n_elems + 15) / 16;
    const int64_t n_spans = (n_chunks + 63) / 64;
    const int64_t n_waves = static_cast<int64_t>(gridDim.x) * WPB;
    const int64_t wave_global = static_cast<int64_t>(blockIdx.x) * WPB + wave;
    const int64_t rounds = (n_spans + n_waves * kScanRound - 1) / (n_waves * kScanRound);
    // distinct (map, threshold) pairs: bit i set = frame i's map is read (wave-uniform, once); `wide` = every such map can be read with
    // aligned 16-byte loads (its pointer + in_off is 16-byte aligned: elem0 and the chunk starts are multiples of 16)
    uint32_t distinct = 0;
    bool wide = (a.elem0 & 15) == 0;
    for (int i = 0; i < a.n_frames; ++i) {
        const uint8_t* d = a.dark[i];
        if (!d) continue;
        bool seen = false;
        for (int k = 0; k < i; ++k) seen = seen || (a.dark[k] == d && a.dark_min[k] == a.dark_min[i]);
        if (seen) continue;
        distinct |= 1u << i;
        wide = wide && (reinterpret_cast<uintptr_t>(d + a.in_off) & 15) == 0;
    }
    const int64_t n_full = a.n_elems / 16;                                  // whole 16-element chunks; a last partial one goes the slow way
    for (int64_t r = 0; r < rounds; ++r) {
        uint32_t hb[kScanRound];
        uint32_t mine = 0;
        if (wide) {
            // no load sits behind a lane-dependent branch: the kScanRound loads of a map are issued back to back (a chunk past the end
            // re-reads chunk 0 and is masked afterwards), then compared
            int64_t off[kScanRound];
            bool valid[kScanRound];
#pragma unroll
            for (int k = 0; k < kScanRound; ++k) {
                const int64_t chunk = (((r * n_waves + wave_global) * kScanRound) + k) * 64 + lane;
                valid[k] = chunk < n_full;
                off[k] = a.in_off + a.elem0 + (valid[k] ? chunk : 0) * 16;
                hb[k] = 0;
            }
            if (n_full > 0) {
                for (uint32_t left = distinct; left; left &= left - 1) {    // wave-uniform loop over the distinct maps
                    const int i = __builtin_amdgcn_readfirstlane(__ffs(static_cast<int>(left)) - 1);
                    const uint8_t* d = a.dark[i];
                    const uint32_t thr = static_cast<uint32_t>(a.dark_min[i]);
                    u32x4 v[kScanRound];
#pragma unroll
                    for (int k = 0; k < kScanRound; ++k) v[k] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(d + off[k]));
#pragma unroll
                    for (int k = 0; k < kScanRound; ++k) {
                        const uint32_t w4[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
                        for (int b = 0; b < 16; ++b) hb[k] |= (((w4[b >> 2] >> (8 * (b & 3))) & 255u) >= thr) ? (1u << b) : 0u;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kScanRound; ++k) {
                const int64_t chunk = (((r * n_waves + wave_global) * kScanRound) + k) * 64 + lane;
                if (!valid[k]) hb[k] = 0;
                if (chunk == n_full && chunk < n_chunks)                    // the tile's last, partial chunk (one lane of one wave)
                    hb[k] = scan_chunk_hotbits(a, a.elem0 + chunk * 16, static_cast<int>(a.n_elems - chunk * 16));
                mine += static_cast<uint32_t>(__popc(hb[k]));
            }
        } else {
#pragma unroll
            for (int k = 0; k < kScanRound; ++k) {
                const int64_t chunk = (((r * n_waves + wave_global) * kScanRound) + k) * 64 + lane;
                hb[k] = 0;
                if (chunk < n_chunks) {
                    const int64_t e0 = a.elem0 + chunk * 16;
                    const int64_t left = a.elem0 + a.n_elems - e0;
                    hb[k] = scan_chunk_hotbits(a, e0, left < 16 ? static_cast<int>(left) : 16);
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
                if (base + total > capacity || base + total < base) {       // queue full: flag it, merge_patch_hot goes over the whole tile instead
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
            uint32_t* q = queue + off;
#pragma unroll
            for (int k = 0; k < kScanRound; ++k) {
                uint32_t bits = hb[k];
                const int64_t chunk = (((r * n_waves + wave_global) * kScanRound) + k) * 64 + lane;
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

int launch_scan_hot(const MergeK& k, uint32_t* ws, uint32_t capacity, hipStream_t st) {
    const int64_t chunks = (k.n_elems + 15) / 16;
    hipLaunchKernelGGL(merge_scan_hot, dim3(stream_grid(chunks, kScanBlock, 1)), dim3(kScanBlock), 0, st, k, ws, capacity);
    return launch_status();
}

// the instantiations the dispatcher links against (hm_merge_host.h declares them extern)
#define HM_INSTANTIATE_HOT(OUT) \
    template int launch_generic<OUT, double>(const MergeK&, bool, bool, hipStream_t); \
    template int launch_fixup<OUT, double>(const MergeK&, bool, bool, hipStream_t); \
    template int launch_hot_queue<OUT, double>(const MergeK&, bool, bool, uint32_t*, size_t, hipStream_t);
HM_INSTANTIATE_HOT(OUT_F64)
HM_INSTANTIATE_HOT(OUT_F32)
#undef HM_INSTANTIATE_HOT

}  // namespace hm
