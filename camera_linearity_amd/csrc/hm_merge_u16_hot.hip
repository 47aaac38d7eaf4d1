// hm_merge_u16_hot.hip - the hot-pixel pass of the uint16 merge (hm_merge_u16_darks; gfx950): uint16 dark maps, frame i hot at an element
// iff (dark DN & M) >= dark_min_dn[i], M = 2^bit_depth - 1. It runs stream-ordered after hm_merge_u16's kernels, which never read a dark
// map, and recomputes the elements that have a hot frame with the k x k medians of the masked DNs (and of the stds) substituted.
//
//   merge_u16_scan_hot    merge_scan_hot for 2-byte maps, the same body (hm_merge_hot_scan_body.h): a lane's chunk of 16 elements is
//                         two 16-byte loads; the queue layout, its piece table and the workspace sizes are the 8-bit pass's.
//   merge_u16_patch_hot   one queued element per lane: merge_u16_element's operation sequence with the medians substituted, every table
//                         gathered from global memory at idx = DN & M (no table in LDS at any depth; LDS holds only the lane's filtered DNs
//                         between the two passes). The queue is dealt as it lies, in blocks of B = ceil(count / waves) <= 64 consecutive
//                         entries per wave (no image-ordered walk through the piece table). With the scan's overflow flag raised, or without
//                         a workspace (queue=0), every lane tests its own elements' dark DNs and patches the hot ones.
//                         LUT (hm_merge_u16_std_table): the stds come from MergeK::std_lut at the filtered DN; a hot frame's is the k x k
//                         median of the mapped neighbourhood, median_j(std_lut[idx_j C + c]) (StdLutDnAt), while icrf_diff is read at the
//                         median DN - the two differ wherever the table is not monotone.
#include "hm_merge_u16.h"

namespace hm {

constexpr int kU16PatchBlock = 256;

__global__ __launch_bounds__(kScanBlock) void merge_u16_scan_hot(const MergeK a, const uint32_t mask, uint32_t* ws, uint32_t capacity) {
    using D = uint16_t;
#include "hm_merge_hot_scan_body.h"
}

// element accessors of the k x k medians: index = (buffer row * W + column) * C + c (lane_median_of, hm_common.h)
struct DnAt {
    const uint16_t* f; uint32_t mask;
    __device__ __forceinline__ uint32_t operator()(int64_t i) const { return static_cast<uint32_t>(f[i]) & mask; }
};

// ... and of the per-DN std table mapped over the same neighbourhood: the std frame the table stands for, never materialised
struct StdLutDnAt {
    const uint16_t* f; uint32_t mask; const double* lut; uint32_t C, c;
    __device__ __forceinline__ double operator()(int64_t i) const { return lut[(static_cast<uint32_t>(f[i]) & mask) * C + c]; }
};

// merge_u16_element's source with the medians of the hot frames substituted: the masked DN of a hot frame is the k x k median of the masked
// DNs around it, its std the k x k median of the std neighbourhood. The neighbourhood is read only where the frame is hot.
// keep: this thread's LDS column (stride kU16PatchBlock) for the filtered DNs between the two passes.
template <bool LUT>
struct U16Filtered {
    const MergeK& a; uint32_t mask; uint16_t* keep; uint32_t hotmask;
    int64_t ei, row, col; int c;
    __device__ __forceinline__ U16Filtered(const MergeK& a_, uint32_t mask_, uint16_t* keep_, int64_t e, uint32_t hotmask_)
        : a(a_), mask(mask_), keep(keep_), hotmask(hotmask_), ei(a_.in_off + e) { elem_to_pixel(a, e, row, col, c); }
    __device__ __forceinline__ uint32_t idx_first(int i) const {
        const uint16_t* f = static_cast<const uint16_t*>(a.frame[i]);
        uint32_t idx = static_cast<uint32_t>(f[ei]) & mask;
        if ((hotmask >> i) & 1u) idx = lane_median_of<uint16_t>(DnAt{f, mask}, a.H, a.W, a.C, a.buf_row0, row, col, c, a.median_k);
        keep[i * kU16PatchBlock] = static_cast<uint16_t>(idx);
        return idx;
    }
    __device__ __forceinline__ uint32_t idx_again(int i) const { return keep[i * kU16PatchBlock]; }
    __device__ __forceinline__ double sd_at(int i) const {
        if constexpr (LUT) {
            const uint32_t C = static_cast<uint32_t>(a.C), cc = static_cast<uint32_t>(c);
            if ((hotmask >> i) & 1u)
                return lane_median_of<double>(StdLutDnAt{static_cast<const uint16_t*>(a.frame[i]), mask, a.std_lut, C, cc}, a.H, a.W, a.C, a.buf_row0,
                                              row, col, c, a.median_k);
            return a.std_lut[keep[i * kU16PatchBlock] * C + cc];           // not hot: the frame's own masked DN
        }
        if ((hotmask >> i) & 1u) return lane_median_of<double>(StdAt<double>{a.sd[i]}, a.H, a.W, a.C, a.buf_row0, row, col, c, a.median_k);
        return a.sd[i][ei];
    }
};

// ws == NULL: no queue (queue=0)
template <bool STD, int OUT, bool LUT = false>
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
            const uint32_t hotmask = lane_hotmask<uint16_t>(a, a.in_off + e, mask);
            if (hotmask) merge_u16_element<STD, OUT>(a, e, U16Filtered<LUT>(a, mask, keep, e, hotmask));
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
            merge_u16_element<STD, OUT>(a, e, U16Filtered<LUT>(a, mask, keep, e, lane_hotmask<uint16_t>(a, a.in_off + e, mask)));
        }
    }
}

int launch_u16_hot(const MergeK& k, int bits, bool with_std, bool lut, bool f32out, uint32_t* ws, size_t ws_bytes, hipStream_t st) {
    if (lut && !with_std) return HM_EINVAL;
    const uint32_t mask = (1u << bits) - 1u;
    if (ws) {
        if (!describe_only("merge_u16_scan_hot")) {
            const size_t head = static_cast<size_t>(kHotQueueHeader) + 2u * hot_piece_slots(k.n_elems);     // counters + piece table, in words
            const size_t words = ws_bytes / 4 - head;                                                       // >= 1 (the caller's size check)
            const uint32_t capacity = static_cast<uint32_t>(words > 0xffffffffull ? 0xffffffffull : words);
            // (the counters were zeroed by the first kernel of this call - MergeK::hot_reset; the scan writes every table entry it owns)
            const int64_t chunks = (k.n_elems + 15) / 16;
            hipLaunchKernelGGL(merge_u16_scan_hot, dim3(stream_grid(chunks, kScanBlock, 1)), dim3(kScanBlock), 0, st, k, mask, ws, capacity);
            const int rc = launch_status();
            if (rc != HM_OK) return rc;
        }
    }
    if (lut ? describe_only(ws ? "merge_u16_patch_hot<bits=%d,std=lut,k=%d>" : "merge_u16_patch_hot<bits=%d,std=lut,k=%d,queue=0>", bits, k.median_k)
            : describe_only(ws ? "merge_u16_patch_hot<bits=%d,std=%d,k=%d>" : "merge_u16_patch_hot<bits=%d,std=%d,k=%d,queue=0>", bits, with_std, k.median_k))
        return HM_OK;
    const unsigned grid = stream_grid(k.n_elems, kU16PatchBlock, ws ? 4 : 8);
    const auto kernel = lut      ? (f32out ? &merge_u16_patch_hot<true, OUT_F32, true> : &merge_u16_patch_hot<true, OUT_F64, true>)
                        : f32out ? (with_std ? &merge_u16_patch_hot<true, OUT_F32> : &merge_u16_patch_hot<false, OUT_F32>)
                                 : (with_std ? &merge_u16_patch_hot<true, OUT_F64> : &merge_u16_patch_hot<false, OUT_F64>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kU16PatchBlock), 0, st, k, mask, static_cast<const uint32_t*>(ws));
    return launch_status();
}

}  // namespace hm
