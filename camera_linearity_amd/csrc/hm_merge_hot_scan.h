// hm_merge_hot_scan.h - the dark-map side of the hot-pixel pass, once for both DN widths (private to the hm_merge*.hip units, on top of
// hm_merge_dev.h): which frames are hot at an element, the hot bits of a 16-element chunk, and the scan that compacts the hot elements into
// the queue of hm_merge_dev.h. Template parameter D is the dark maps' DN type: uint8_t (hm_merge*: mask = the literal 255) or uint16_t
// (hm_merge_u16_darks: the maps travel in MergeK::dark, typed const uint8_t*, and are read through dark_as<uint16_t>(); mask =
// 2^bit_depth - 1). Frame i is hot at an element iff (dark DN & mask) >= dark_min[i]. The scan itself is hm_merge_hot_scan_body.h, the one
// text that is the body of merge_scan_hot (hm_merge_hot.hip) and of merge_u16_scan_hot (hm_merge_u16_hot.hip).
#pragma once
#include "hm_merge_dev.h"

namespace hm {

constexpr int kScanRound = 4;           // chunks of 16 elements a lane scans per round: 65 536 elements per workgroup and round
constexpr int kScanBlock = 1024;

template <typename D>
__host__ __device__ __forceinline__ const D* dark_as(const MergeK& a, int i) { return reinterpret_cast<const D*>(a.dark[i]); }

// frames that are hot at input element ei: bit i
template <typename D>
__device__ __forceinline__ uint32_t lane_hotmask(const MergeK& a, int64_t ei, uint32_t mask) {
    uint32_t hotmask = 0;
    const int N = a.n_frames;
    for (int i0 = 0; i0 < N; i0 += 8) {
        uint32_t d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            d[k] = 0;
            if (i0 + k < N && a.dark[i0 + k]) d[k] = dark_as<D>(a, i0 + k)[ei];              // wave-uniform condition
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)                                  // (a 1-byte DN has no bit to mask; `& 255u` spelled out survives as an instruction)
            if (i0 + k < N && a.dark[i0 + k])
                hotmask |= (static_cast<int>(sizeof(D) == 1 ? d[k] : d[k] & mask) >= a.dark_min[i0 + k]) ? (1u << (i0 + k)) : 0u;
    }
    return hotmask;
}

// `if (frame i's (map d, threshold) is an earlier frame's) continue;`: every DISTINCT pair is read once (the d * N term of the algorithmic
// bytes). Text, not a function, for the reason hm_merge_hot_scan_body.h gives: as an inlined function it moved merge_fixup_hot's instructions.
#define HM_SKIP_REPEATED_DARK(a, i, d) \
    bool seen = false; \
    for (int k = 0; k < i; ++k) seen = seen || (dark_as<D>(a, k) == d && a.dark_min[k] == a.dark_min[i]); \
    if (seen) continue;

// hot bits of a chunk of cnt <= 16 elements starting at e0 (relative to row0): bit b set iff element e0 + b is hot in at least one frame.
// One load per element and map: maps that are not 16-byte aligned at the tile's first element, and the tile's last, partial chunk - but a
// whole chunk of a 1-byte map that is aligned takes one 16-byte load (merge_fixup_hot scans with this function alone).
template <typename D>
__device__ __forceinline__ uint32_t scan_chunk_hotbits(const MergeK& a, uint32_t mask, int64_t e0, int cnt) {
    uint32_t hotbits = 0;
    for (int i = 0; i < a.n_frames; ++i) {
        const D* d = dark_as<D>(a, i);
        if (!d) continue;
        HM_SKIP_REPEATED_DARK(a, i, d)
        const D* p = d + a.in_off + e0;
        const uint32_t thr = static_cast<uint32_t>(a.dark_min[i]);
        if (sizeof(D) == 1 && cnt == 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int b = 0; b < 16; ++b) hotbits |= (((w4[b >> 2] >> (8 * (b & 3))) & mask) >= thr) ? (1u << b) : 0u;   // (1-byte DNs)
        } else {
            for (int b = 0; b < cnt; ++b) hotbits |= ((static_cast<uint32_t>(p[b]) & mask) >= thr) ? (1u << b) : 0u;
        }
    }
    return hotbits;
}

}  // namespace hm
