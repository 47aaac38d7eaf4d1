// hm_merge_u16.h - what the two units of the uint16 merge share (private to hm_merge_u16.hip and hm_merge_u16_hot.hip): the masked DN
// load and the hot-pixel pass's launcher. A uint16 dark map travels in MergeK::dark (typed const uint8_t*: the struct keeps its layout)
// and is read through dark16(); its threshold, 1 .. 2^bit_depth, in MergeK::dark_min.
#pragma once
#include "hm_merge_host.h"

namespace hm {

__device__ __forceinline__ uint32_t ld_dn16(const MergeK& a, int i, int64_t ei, uint32_t mask) {
    return static_cast<uint32_t>(static_cast<const uint16_t*>(a.frame[i])[ei]) & mask;
}
__host__ __device__ __forceinline__ const uint16_t* dark16(const MergeK& a, int i) { return reinterpret_cast<const uint16_t*>(a.dark[i]); }

// hm_merge_u16_hot.hip: the stream-ordered pass after hm_merge_u16's kernels (hm_merge_u16_darks). ws != NULL: merge_u16_scan_hot queues
// the hot elements in the workspace (counters zeroed by the call's first kernel through MergeK::hot_reset) and merge_u16_patch_hot
// recomputes one queued element per lane; ws == NULL: merge_u16_patch_hot tests every element's dark DNs itself (queue=0).
int launch_u16_hot(const MergeK& k, int bits, bool with_std, bool f32out, uint32_t* ws, size_t ws_bytes, hipStream_t st);

}  // namespace hm
