// hm_merge_rules.h - the argument rules of the fused merge's six C entry points (hm_merge, hm_merge_std_table, hm_merge_std_f32, hm_merge_u16,
// hm_merge_u16_darks, hm_merge_u16_std_table), written
// once for both builds of the ABI: the device build's dispatcher (hm_merge.hip) and the host build (csrc_host/hm_host.cpp) include this file
// and hold no argument test of their own - one ABI, one answer. Plain C++17 on hdrmerge.h and the standard headers: no HIP type, no OpenMP.
//
// What lives here: the struct_size values accepted and their widening, where a call's stds come from, every status a call can be refused
// with - in the order the specification gives them: an earlier rule wins over a later one broken in the same call - and the algorithmic byte
// count. What a build does with a validated call (MergeCall) is its own business.
//
// The one difference between the builds: a table call (hm_merge_std_table) with more than HM_MAX_FRAMES frames or variant <= -2 is
// HM_EUNSUPPORTED on the device build, whose chunked path reads std frames (hm_merge.hip adds that refusal after check_merge_call), and runs
// on the host build, which takes any number of frames in one pass. The device build's only other addition refuses what a tuning build
// (-DHM_TUNE_NF) has no float32-output instantiations for.
#pragma once
#include "hdrmerge.h"
#include <cstdint>
#include <cstring>

namespace hm_rules {

enum MergeEntry { ENTRY_MERGE, ENTRY_STD_TABLE, ENTRY_STD_F32, ENTRY_U16, ENTRY_U16_DARKS, ENTRY_U16_STD_TABLE };   // the C entry point called
constexpr bool entry_is_u16(MergeEntry e) { return e == ENTRY_U16 || e == ENTRY_U16_DARKS || e == ENTRY_U16_STD_TABLE; }

// hm_merge_u16's own arguments (check_merge_call's `extra` for ENTRY_U16), hm_merge_u16_darks's (ENTRY_U16_DARKS: with the N dark maps) and
// hm_merge_u16_std_table's (ENTRY_U16_STD_TABLE: with the (2^bit_depth, C) per-DN std table, and the N dark maps or NULL for no hot-pixel pass)
struct U16Extra { const uint16_t* const* frames; int bit_depth; const uint16_t* const* darks = nullptr; const double* std_table = nullptr; };

// hm_merge_u16: which of a call's tables a streaming kernel holds in LDS, the bytes that takes, and the fit rule - at most a gfx950
// workgroup's 160 KiB (hdrmerge.h states all of it for callers). n = 2^bit_depth rows:
//   U16_TAB_ALL     value-only w[n] | (w g)[n C]: 8 (1 + C) n bytes; with std {w, dw}[n] | {g, d}[n C]: 16 (1 + C) n bytes
//   U16_TAB_WDW_G   (std calls) {w, dw}[n] | g[n C]: 8 (2 + C) n bytes; icrf_diff is gathered from global memory. In a table call
//                   (hm_merge_u16_std_table) the same bytes hold {w, dw}[n] | dg[n C], dg = icrf_diff * std_table, and icrf is gathered
//   U16_TAB_PER_DN  the per-DN tables only - w[n]: 8 n bytes, with std {w, dw}[n]: 16 n bytes; the per-(DN, channel) ones from global memory
//   U16_TAB_GLOBAL  nothing in LDS
enum U16Tables { U16_TAB_GLOBAL = 0, U16_TAB_PER_DN = 1, U16_TAB_WDW_G = 2, U16_TAB_ALL = 3 };
constexpr int64_t kU16MaxLds = 160 * 1024;
inline int64_t u16_table_bytes(int bit_depth, int C, bool with_std, int place = U16_TAB_ALL) {
    const int64_t n = int64_t{1} << bit_depth;
    switch (place) {
        case U16_TAB_ALL: return (with_std ? 16 : 8) * int64_t{1 + C} * n;
        case U16_TAB_WDW_G: return 8 * int64_t{2 + C} * n;
        case U16_TAB_PER_DN: return (with_std ? 16 : 8) * n;
        default: return 0;
    }
}
inline bool u16_tables_fit_lds(int bit_depth, int C, bool with_std) { return u16_table_bytes(bit_depth, C, with_std) <= kU16MaxLds; }
// the largest PARTIAL placement that fits (variant 3; the library's choice where not everything fits), U16_TAB_GLOBAL when none does
inline int u16_mixed_tables(int bit_depth, int C, bool with_std) {
    if (with_std && u16_table_bytes(bit_depth, C, true, U16_TAB_WDW_G) <= kU16MaxLds) return U16_TAB_WDW_G;
    return u16_table_bytes(bit_depth, C, with_std, U16_TAB_PER_DN) <= kU16MaxLds ? U16_TAB_PER_DN : U16_TAB_GLOBAL;
}

// where the call's per-frame stds come from
enum StdSource {
    STD_NONE,     // no std is formed (a std-entry call without out_val too: it is hm_merge's sum-of-weights call)
    STD_F64,      // args->stds: N float64 frames
    STD_TABLE,    // hm_merge_std_table: the (256, C) per-DN table, hm_merge_u16_std_table: the (2^bit_depth, C) one; args->stds is NULL
    STD_F32       // hm_merge_std_f32: N float32 frames, 4-byte aligned; MergeCall::a.stds addresses them
};

// A call that passed check_merge_call().
struct MergeCall {
    hm_merge_args a;                   // the caller's arguments in the current layout
    StdSource std_src;
    const double* std_table;           // STD_TABLE: the table, else NULL
    bool f64in;                        // float64 frames (else uint8, or uint16 in a hm_merge_u16 call)
    const uint16_t* const* frames_u16; // hm_merge_u16: the N frames (a.frames_u8 and a.frames_f64 are NULL), else NULL
    int bit_depth;                     // hm_merge_u16: 9..16, else 0
    const uint16_t* const* darks_u16;  // hm_merge_u16_darks, hm_merge_u16_std_table with maps: the N dark maps (NULL entries: no filter; a.darks_u8 is NULL), else NULL
    bool with_std;                     // std_src != STD_NONE
    bool flat;                         // a flat field of either kind
    bool hot;                          // at least one frame has a dark map
    bool f32out;                       // out_kind == HM_OUT_F32
    bool empty;                        // rows == 0: nothing to do; none of the rules after the shape of the tile has been looked at
};

inline bool ptr_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// struct_size values hm_merge accepts: the current layout and the two older ones of ABI version 1 (without the hot-pixel queue
// workspace: 264 bytes; with it: 280 bytes) - the missing tail reads as zero (no workspace). out_kind took the place of a pad word those
// callers never promised to zero: for them it is cleared (float64 outputs).
inline bool widen_args(const hm_merge_args* g, hm_merge_args& full) {
    if (!g) return false;
    const uint32_t sz = g->struct_size;
    if (sz != sizeof(hm_merge_args) && sz != 264u && sz != 280u) return false;
    full = hm_merge_args{};
    std::memcpy(&full, g, sz < sizeof(hm_merge_args) ? sz : sizeof(hm_merge_args));
    if (sz != sizeof(hm_merge_args)) full.out_kind = HM_OUT_F64;
    full.struct_size = sizeof(hm_merge_args);
    return true;
}

// extra: the entry point's own pointer - NULL for hm_merge, std_table for hm_merge_std_table, stds_f32 for hm_merge_std_f32, a U16Extra
// for hm_merge_u16, hm_merge_u16_darks and hm_merge_u16_std_table.
// Returns the call's status; `call` is complete when that is HM_OK (with call.empty set there is nothing to run).
inline int check_merge_call(const hm_merge_args* g_in, MergeEntry entry, const void* extra, MergeCall& call) {
    call = MergeCall{};
    if (!widen_args(g_in, call.a)) return HM_EINVAL;
    hm_merge_args* const g = &call.a;
    const int N = g->n_frames, C = g->channels;
    // the std entries' own rules; without out_val they form no std and the call is hm_merge's
    if (entry == ENTRY_STD_TABLE) {
        const double* std_table = static_cast<const double*>(extra);
        if (g->stds || !std_table || !g->icrf_diff) return HM_EINVAL;
        if (g->frames_u8 && !g->dw_lut) return HM_EINVAL;
        if (g->out_val && !g->out_std) return HM_EINVAL;
        if (!ptr_aligned(std_table, 8)) return HM_EALIGN;
        if (g->out_val) { call.std_src = STD_TABLE; call.std_table = std_table; }
    } else if (entry == ENTRY_STD_F32) {
        const float* const* stds_f32 = static_cast<const float* const*>(extra);
        if (g->stds || !stds_f32) return HM_EINVAL;
        for (int i = 0; i < N; ++i)
            if (!stds_f32[i]) return HM_EINVAL;
        if (!g->icrf_diff) return HM_EINVAL;
        if (g->frames_u8 && !g->dw_lut) return HM_EINVAL;
        if (g->out_val && !g->out_std) return HM_EINVAL;
        for (int i = 0; i < N; ++i)
            if (!ptr_aligned(stds_f32[i], 4)) return HM_EALIGN;
        if (g->out_val) { call.std_src = STD_F32; g->stds = reinterpret_cast<const double* const*>(stds_f32); }
    } else if (entry_is_u16(entry)) {
        const U16Extra* x = static_cast<const U16Extra*>(extra);
        const bool table = entry == ENTRY_U16_STD_TABLE;
        // the maps of a call: hm_merge_u16_darks always has them, hm_merge_u16_std_table may
        const bool darks = entry == ENTRY_U16_DARKS || (table && x && x->darks);
        if (g->frames_u8 || g->frames_f64 || !x || !x->frames) return HM_EINVAL;
        for (int i = 0; i < N; ++i)
            if (!x->frames[i]) return HM_EINVAL;
        if (x->bit_depth < 9 || x->bit_depth > 16 || !g->w_lut) return HM_EINVAL;
        if (g->stds && (!g->icrf_diff || !g->dw_lut)) return HM_EINVAL;
        // hm_merge_u16_std_table: the table takes the place of the std frames (hm_merge_std_table's rules)
        if (table && (g->stds || !x->std_table || !g->icrf_diff || !g->dw_lut)) return HM_EINVAL;
        if (table && g->out_val && !g->out_std) return HM_EINVAL;
        // the maps come beside the struct (uint16), never in it (uint8), and always with their thresholds
        if (darks && (!x->darks || g->darks_u8 || !g->dark_min_dn)) return HM_EINVAL;
        for (int i = 0; i < N; ++i)
            if (!ptr_aligned(x->frames[i], 2)) return HM_EALIGN;
        if (darks) {
            for (int i = 0; i < N; ++i)
                if (!ptr_aligned(x->darks[i], 2)) return HM_EALIGN;
            call.darks_u16 = x->darks;
        }
        if (table && !ptr_aligned(x->std_table, 8)) return HM_EALIGN;
        call.frames_u16 = x->frames; call.bit_depth = x->bit_depth;
        if (g->stds) call.std_src = STD_F64;
        if (table && g->out_val) { call.std_src = STD_TABLE; call.std_table = x->std_table; }   // (without out_val: hm_merge_u16's sum-of-weights call)
    } else if (g->stds) call.std_src = STD_F64;
    // hm_merge's rules
    if (N < 1 || C < 1 || g->height < 1 || g->width < 1 || g->rows < 0) return HM_EINVAL;
    if (g->out_kind != HM_OUT_F64 && g->out_kind != HM_OUT_F32) return HM_EINVAL;
    call.f32out = g->out_kind == HM_OUT_F32;
    if (C > HM_MAX_CHANNELS) return HM_EUNSUPPORTED;
    if (g->rows == 0) {                                                  // empty tile: nothing to do
        call.empty = true;
        return g->row0 >= 0 && g->row0 <= g->height ? HM_OK : HM_ESHAPE;
    }
    call.f64in = g->frames_f64 != nullptr;
    if (!call.frames_u16 && call.f64in == (g->frames_u8 != nullptr)) return HM_EINVAL;       // exactly one input kind
    if (!g->exposures || !g->icrf) return HM_EINVAL;
    const bool with_std = call.with_std = call.std_src != STD_NONE;
    if (!g->out_val && !g->out_sum_w) return HM_EINVAL;
    if (g->out_val) {
        if (with_std != (g->out_std != nullptr)) return HM_EINVAL;
        if (with_std && !g->icrf_diff) return HM_EINVAL;
    }
    if (!call.f64in && (!g->w_lut || (with_std && !g->dw_lut))) return HM_EINVAL;
    call.flat = g->flat_u8 || g->flat_f64;
    if (g->flat_u8 && g->flat_f64) return HM_EINVAL;
    if (call.flat && with_std && !g->flat_std) return HM_EINVAL;
    // geometry
    if (g->row0 < 0 || g->row0 + g->rows > g->height) return HM_ESHAPE;
    if (g->buf_row0 < 0 || g->buf_row0 > g->row0 || g->buf_row0 + g->buf_rows > g->height ||
        g->buf_row0 + g->buf_rows < g->row0 + g->rows) return HM_ESHAPE;
    if (g->darks_u8) {
        if (!g->dark_min_dn) return HM_EINVAL;
        for (int i = 0; i < N; ++i) call.hot = call.hot || (g->darks_u8[i] != nullptr);
    }
    if (call.darks_u16)
        for (int i = 0; i < N; ++i) call.hot = call.hot || (call.darks_u16[i] != nullptr);
    if (call.hot) {
        const int k = g->median_k;
        if (k < 3 || k > 7 || (k % 2) == 0) return HM_EINVAL;
        const int64_t r = k / 2;
        const int64_t need_lo = g->row0 - r < 0 ? 0 : g->row0 - r;
        const int64_t need_hi = g->row0 + g->rows + r > g->height ? g->height : g->row0 + g->rows + r;
        if (g->buf_row0 > need_lo || g->buf_row0 + g->buf_rows < need_hi) return HM_ESHAPE;   // halo too small
        // hm_merge_u16_darks: the threshold of every frame that has a map, 1 .. 2^bit_depth (2^bit_depth: no DN is hot)
        if (call.darks_u16)
            for (int i = 0; i < N; ++i)
                if (call.darks_u16[i] && (g->dark_min_dn[i] < 1 || g->dark_min_dn[i] > (1 << call.bit_depth))) return HM_EINVAL;
    }
    // per-frame pointers and exposures (any N: neither build's hm_merge has a frame limit)
    for (int i = 0; i < N; ++i) {
        const void* f = call.frames_u16 ? static_cast<const void*>(call.frames_u16[i])
                        : call.f64in ? static_cast<const void*>(g->frames_f64[i]) : static_cast<const void*>(g->frames_u8[i]);
        if (!f) return HM_EINVAL;
        if (call.f64in && !ptr_aligned(f, 8)) return HM_EALIGN;
        if (g->stds) {
            if (!g->stds[i]) return HM_EINVAL;
            if (!ptr_aligned(g->stds[i], call.std_src == STD_F32 ? 4 : 8)) return HM_EALIGN;
        }
        if (!(g->exposures[i] > 0.0)) return HM_EINVAL;
    }
    const int out_align = call.f32out ? 4 : 8;
    if ((g->out_val && !ptr_aligned(g->out_val, out_align)) || (g->out_std && !ptr_aligned(g->out_std, out_align)) ||
        (g->out_sum_w && !ptr_aligned(g->out_sum_w, 8))) return HM_EALIGN;
    // What only the device build's one-launch kernels have, refused by both builds so that a call means the same on both: float32 outputs
    // (the chunked path keeps float64 running sums in out_val / out_std and the row-band loop advances output pointers by float64 elements)
    // and float32 std frames (the chunked path reads float64 ones).
    const bool chunked = N > HM_MAX_FRAMES || g->variant <= -2;
    if (call.f32out && (chunked || g->rows * g->width * static_cast<int64_t>(C) >= (int64_t{1} << 32))) return HM_EUNSUPPORTED;
    if (call.std_src == STD_F32 && chunked) return HM_EUNSUPPORTED;
    if (entry_is_u16(entry)) {
        // variant: 0 the library's choice, -1 one element per thread, 1 / 2 / 3 the streaming kernel with its tables in LDS / in global
        // memory / split between the two (the largest partial placement)
        if (g->variant > 3) return HM_EINVAL;
        // what the uint16 entries leave out: uint8 dark maps and uint8 flat fields (8-bit data), the chunked path
        if (g->darks_u8 || g->flat_u8 || chunked) return HM_EUNSUPPORTED;
        if (g->variant == 1 && !u16_tables_fit_lds(call.bit_depth, C, with_std && g->out_val)) return HM_EUNSUPPORTED;
        if (g->variant == 3 && u16_mixed_tables(call.bit_depth, C, with_std && g->out_val) == U16_TAB_GLOBAL) return HM_EUNSUPPORTED;
    }
    return HM_OK;
}

// Algorithmic bytes of a call through `entry` (hdrmerge.h: hm_merge_algorithmic_bytes): STD_TABLE calls read no std stream, STD_F32 calls
// 4-byte ones (args->stds is NULL in both). Takes the caller's arguments as they are: a refused call has a count too.
// darks_u16 (ENTRY_U16_DARKS, ENTRY_U16_STD_TABLE): the N uint16 dark maps, 2 bytes per element for every distinct (map, threshold).
inline int64_t merge_algorithmic_bytes(const hm_merge_args* g, MergeEntry entry, const uint16_t* const* darks_u16 = nullptr) {
    if (!g || g->n_frames <= 0 || g->rows <= 0 || g->width <= 0 || g->channels <= 0) return 0;
    const int64_t E = g->rows * g->width * g->channels;
    const int N = g->n_frames;
    const bool lut = entry == ENTRY_STD_TABLE || entry == ENTRY_U16_STD_TABLE, sd32 = entry == ENTRY_STD_F32;
    const bool s = lut || sd32 || g->stds != nullptr;
    const int64_t in_b = entry_is_u16(entry) ? 2 : g->frames_f64 ? 8 : 1;
    int64_t per = N * (in_b + ((s && !lut) ? (sd32 ? 4 : 8) : 0));
    const bool f32out = g->struct_size == sizeof(hm_merge_args) && g->out_kind == HM_OUT_F32;   // (the older layouts have no out_kind)
    if (g->out_val) per += (f32out ? 4 : 8) * (1 + (s ? 1 : 0));
    if (g->out_sum_w) per += 8;
    if (g->flat_u8 || g->flat_f64) per += (g->flat_u8 ? 1 : 8) + ((s && g->flat_std) ? 8 : 0);
    if (g->darks_u8)                                       // every DISTINCT (map, threshold) is read once (the device build's scan)
        for (int i = 0; i < N; ++i) {
            if (!g->darks_u8[i]) continue;
            bool seen = false;
            for (int k = 0; k < i; ++k)
                seen = seen || (g->darks_u8[k] == g->darks_u8[i] && (!g->dark_min_dn || g->dark_min_dn[k] == g->dark_min_dn[i]));
            per += seen ? 0 : 1;
        }
    if ((entry == ENTRY_U16_DARKS || entry == ENTRY_U16_STD_TABLE) && darks_u16)
        for (int i = 0; i < N; ++i) {
            if (!darks_u16[i]) continue;
            bool seen = false;
            for (int k = 0; k < i; ++k)
                seen = seen || (darks_u16[k] == darks_u16[i] && (!g->dark_min_dn || g->dark_min_dn[k] == g->dark_min_dn[i]));
            per += seen ? 0 : 2;
        }
    return per * E;
}

}  // namespace hm_rules
