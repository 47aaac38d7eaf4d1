// hm_merge_u16.h - what the two units of the uint16 merge share (private to hm_merge_u16.hip and hm_merge_u16_hot.hip): the masked DN
// load, the per-element operation sequence and the hot-pixel pass's launcher. A uint16 dark map travels in MergeK::dark (typed
// const uint8_t*: the struct keeps its layout) and is read through dark_as<uint16_t>() (hm_merge_hot_scan.h); its threshold,
// 1 .. 2^bit_depth, in MergeK::dark_min.
#pragma once
#include "hm_merge_host.h"
#include "hm_merge_hot_scan.h"

namespace hm {

__device__ __forceinline__ uint32_t ld_dn16(const MergeK& a, int i, int64_t ei, uint32_t mask) {
    return static_cast<uint32_t>(static_cast<const uint16_t*>(a.frame[i])[ei]) & mask;
}

// merge_one_element<false, STD, HOT_NONE, OUT> for uint16 frames, tables in global memory. SRC says where frame i's table index and std
// come from (the host build's idx_at / sd_at): c = the element's channel; idx_first(i) in the S pass, idx_again(i) in the second pass,
// sd_at(i) there in std calls. U16Frames below reads the frames as they are; the hot-pixel pass substitutes the k x k medians of the hot
// frames (U16Filtered, hm_merge_u16_hot.hip) - the same operations in the same order, so the same bits on pre-filtered frames.
template <bool STD, int OUT, typename SRC>
__device__ __forceinline__ void merge_u16_element(const MergeK& a, int64_t e, const SRC& src) {
    const int C = a.C, N = a.n_frames, c = src.c;
    double S = 0.0;
    for (int i = 0; i < N; ++i) {
        const double w = a.w_lut[src.idx_first(i)];
        S = (i == 0) ? w : S + w;                                       // exposure_series.py:340
    }
    if (a.out_sum_w) a.out_sum_w[e] = S;
    if (!a.out_val) return;
    const double invS = 1.0 / S;
    const double invS2 = 1.0 / (S * S);                                 // 1 / S**2, exposure_series.py:343
    double acc = 0.0, var = 0.0;
    for (int i = 0; i < N; ++i) {
        const uint32_t idx = src.idx_again(i);
        const double w = a.w_lut[idx];
        const double dw = STD ? a.dw_lut[idx] : 0.0;
        const double g = a.icrf[idx * C + c];
        const double it = a.inv_t[i];
        const double wg = w * g;
        acc = (i == 0) ? wg * it : fma(wg, it, acc);                    // :388 numerator
        if (STD) {
            const double dg = a.icrf_diff[idx * C + c] * src.sd_at(i);  // measurand.py:512
            const double term = merge_var_term(w, dw, g, dg, invS, invS2, it);   // :389
            var = (i == 0) ? term * term : fma(term, term, var);
        }
    }
    double val = acc / S;
    double sd = STD ? sqrt(var) : 0.0;                                  // :394
    if (a.has_flat) flat_field_apply(a, e, c, STD, val, sd);            // (flat_u8 is NULL in these calls: the float64 flat field)
    store_out<OUT>(a.out_val, e, val);
    if (STD) store_out<OUT>(a.out_std, e, sd);
}

struct U16Frames {
    const MergeK& a; uint32_t mask; int64_t ei; int c;
    __device__ __forceinline__ U16Frames(const MergeK& a_, uint32_t mask_, int64_t e) : a(a_), mask(mask_), ei(a_.in_off + e), c(static_cast<int>(e % a_.C)) {}
    __device__ __forceinline__ uint32_t idx_first(int i) const { return ld_dn16(a, i, ei, mask); }
    __device__ __forceinline__ uint32_t idx_again(int i) const { return ld_dn16(a, i, ei, mask); }
    __device__ __forceinline__ double sd_at(int i) const { return a.sd[i][ei]; }
};

// hm_merge_u16_std_table: frame i's std is the per-DN table's entry at the frame's own masked DN (MergeK::std_lut, (2^bit_depth, C))
struct U16FramesLut : U16Frames {
    using U16Frames::U16Frames;
    __device__ __forceinline__ double sd_at(int i) const { return a.std_lut[ld_dn16(a, i, ei, mask) * static_cast<uint32_t>(a.C) + static_cast<uint32_t>(c)]; }
};

// hm_merge_u16_hot.hip: the stream-ordered pass after hm_merge_u16's kernels (hm_merge_u16_darks). ws != NULL: merge_u16_scan_hot queues
// the hot elements in the workspace (counters zeroed by the call's first kernel through MergeK::hot_reset) and merge_u16_patch_hot
// recomputes one queued element per lane; ws == NULL: merge_u16_patch_hot tests every element's dark DNs itself (queue=0).
// lut (with_std only): the stds come from k.std_lut, a hot frame's as the median of the mapped neighbourhood.
int launch_u16_hot(const MergeK& k, int bits, bool with_std, bool lut, bool f32out, uint32_t* ws, size_t ws_bytes, hipStream_t st);

}  // namespace hm
