// hm_merge_u16.hip - the fused merge for 9- to 16-bit cameras (gfx950): uint16 DN frames, an explicit bit depth, per-DN tables of
// 2^bit_depth rows (hdrmerge.h: hm_merge_u16). The kernel map of the 8-bit merge is in hm_merge.hip; this unit holds its own family, the
// dispatch and the C entry points. The argument rules are hm_merge_rules.h's ENTRY_U16 (shared with the host build).
//
//   merge_u16_generic   one element per thread, tables gathered from global memory: any alignment, the tails, variant = -1, the
//                       sum-of-weights-only call. merge_generic with 2-byte loads and table pointers that address global memory.
//   merge_u16_stream    merge_u8_loop / merge_u8_loop_std's decomposition at run-time N and C: a wave owns groups of 128 consecutive
//                       elements, a lane two of them - one 4-byte load per frame, 16-byte stores - frames in chunks of kU16Chunk.
//                       Template parameter PLACE (hm_rules::U16Tables) says where the tables live:
//                         tab=lds     dynamic LDS, value-only w[2^b] | (w g)[2^b C] (8 (1 + C) 2^b bytes), with std {w, dw}[2^b] |
//                                     {g, d}[2^b C] (16 (1 + C) 2^b bytes); chosen when that is at most 160 KiB (hm_rules::u16_tables_fit_lds).
//                                     One workgroup of 1024 threads owns the CU (16 waves cover the gather latency; __launch_bounds__(1024)
//                                     keeps the kernel at 128 registers); the grid is no larger than the number of 16-group blocks of the
//                                     call, so a small image does not fill a table per CU for nothing.
//                         tab=mixed-wdwg / mixed-wdw / mixed-w   the largest part that fits where not everything does: {w, dw} and g
//                                     (std calls; icrf_diff gathered from global memory), or the per-DN tables alone ({w, dw} / w; the
//                                     per-(DN, channel) tables from global memory). Same workgroup shape as tab=lds.
//                         tab=global  the same loop with every gather going through L1 / L2: what is left (16 bits always).
// Every table access - LDS or global - is at idx = DN & (2^bit_depth - 1): stray high bits never read outside a table.
// One operation sequence per output element in every kernel, merge_one_element's (hm_merge_dev.h): S in frame order, 1/S and 1/S**2 once,
// the numerator and the variance terms accumulated with fma in frame order, the product w g formed once (a table entry or a register).
// hm_merge_u16_darks adds the hot-pixel pass of hm_merge_u16_hot.hip after these kernels (ENTRY_U16_DARKS): they never read a dark map; the
// first of them zeroes the hot-pixel queue's counters in passing (MergeK::hot_reset, NULL in every hm_merge_u16 call).
// The kernel text and the launchers are hm_merge_u16_kernels.h; this unit instantiates them for value-only calls and float64 std frames,
// hm_merge_u16_lut.hip for the per-DN std table (hm_merge_u16_std_table, ENTRY_U16_STD_TABLE: "std=lut", tab=mixed-wdwdg).
#include "hm_merge_u16_kernels.h"

namespace hm {

// The library's choice of the table placement (variant = 0): everything in LDS where it fits, else the largest part that does
// (measured: DESIGN.md 4.1.5).
static int u16_default_tables(int bits, int C, bool with_std) {
    return hm_rules::u16_tables_fit_lds(bits, C, with_std) ? hm_rules::U16_TAB_ALL : hm_rules::u16_mixed_tables(bits, C, with_std);
}

template <int OUT>
static int merge_u16_launch(const hm_rules::MergeCall& call, void* stream) {
    const hm_merge_args* g = &call.a;
    const int N = g->n_frames, C = g->channels, bits = call.bit_depth;
    const bool with_std = call.with_std && g->out_val, flat = call.flat, hot = call.hot;
    MergeK k{};
    for (int i = 0; i < N; ++i) {
        k.frame[i] = call.frames_u16[i];
        if (g->stds) k.sd[i] = g->stds[i];
        k.inv_t[i] = 1.0 / g->exposures[i];
        k.dark[i] = hot ? reinterpret_cast<const uint8_t*>(call.darks_u16[i]) : nullptr;       // read through dark_as<uint16_t>()
        k.dark_min[i] = hot && call.darks_u16[i] ? g->dark_min_dn[i] : 1 << 16;
    }
    k.icrf = g->icrf; k.icrf_diff = g->icrf_diff; k.w_lut = g->w_lut; k.dw_lut = g->dw_lut;
    k.std_lut = with_std ? call.std_table : nullptr;       // hm_merge_u16_std_table: the LUT instantiations (hm_merge_u16_lut.hip)
    const bool lut = k.std_lut != nullptr;
    k.flat_f64 = g->flat_f64; k.flat_std = g->flat_std;
    for (int c = 0; c < HM_MAX_CHANNELS; ++c) { k.ff_mean[c] = g->ff_mean[c]; k.ff_std_mean[c] = g->ff_std_mean[c]; }
    k.out_val = g->out_val; k.out_std = g->out_std; k.out_sum_w = g->out_sum_w;
    const int64_t E = g->rows * g->width * C;
    k.n_elems = E; k.elem0 = 0;
    k.in_off = (g->row0 - g->buf_row0) * g->width * C;
    k.H = g->height; k.W = g->width; k.row0 = g->row0; k.buf_row0 = g->buf_row0; k.buf_rows = g->buf_rows;
    k.n_frames = N; k.C = C; k.median_k = hot ? g->median_k : 3; k.has_flat = flat ? 1 : 0;
    k.variant = g->variant; k.inv_t_inrange = 1;
    hipStream_t st = as_stream(stream);
    // the hot-pixel pass's queue: the caller's workspace where it is usable (hm_merge's rule), else the pass tests every element itself
    const bool hot_queue = hot && g->hot_workspace && g->hot_workspace_bytes >= hm_merge_hot_workspace_min_bytes(E) &&
                           aligned(g->hot_workspace, 16) && E < (int64_t{1} << 32);
    k.hot_reset = hot_queue ? static_cast<uint32_t*>(g->hot_workspace) : nullptr;
    const auto hot_pass = [&]() {
        if (!hot) return static_cast<int>(HM_OK);
        return launch_u16_hot(k, bits, with_std, lut, OUT == OUT_F32, hot_queue ? static_cast<uint32_t*>(g->hot_workspace) : nullptr,
                              hot_queue ? g->hot_workspace_bytes : 0, st);
    };

    // the pair rule (hdrmerge.h): 4-byte frame words, 16-byte float64 pairs (8-byte float32 ones)
    bool fast = g->out_val && E < (int64_t{1} << 32) && g->variant >= 0;
    for (int i = 0; i < N && fast; ++i) {
        fast = aligned(call.frames_u16[i] + k.in_off, 4);
        if (fast && with_std && !lut) fast = aligned(k.sd[i] + k.in_off, 16);
    }
    constexpr int pair_bytes = OUT == OUT_F32 ? 8 : 16;
    fast = fast && aligned(k.out_val, pair_bytes) && (!k.out_std || aligned(k.out_std, pair_bytes)) && (!k.out_sum_w || aligned(k.out_sum_w, 16));
    if (fast && flat) fast = aligned(k.flat_f64, 16) && (!with_std || aligned(k.flat_std, 16));
    const auto generic = [&](const MergeK& kk) {
        return lut ? launch_u16_generic<OUT, true>(kk, bits, with_std, st) : launch_u16_generic<OUT, false>(kk, bits, with_std, st);
    };
    if (!fast) {
        const int rc = generic(k);
        return rc != HM_OK ? rc : hot_pass();
    }

    // (variants 1 and 3 that do not fit: refused by the rules)
    const int place = g->variant == 1 ? hm_rules::U16_TAB_ALL : g->variant == 2 ? hm_rules::U16_TAB_GLOBAL
                      : g->variant == 3 ? hm_rules::u16_mixed_tables(bits, C, with_std) : u16_default_tables(bits, C, with_std);
    const int64_t body = (E / kSub) * kSub;
    if (body > 0) {
        MergeK kb = k;
        kb.n_elems = body;
        const int rc = lut ? launch_u16_stream<OUT, true>(kb, bits, with_std, place, st) : launch_u16_stream<OUT, false>(kb, bits, with_std, place, st);
        if (rc != HM_OK) return rc;
    }
    if (body < E) {                                        // tail: less than one group
        MergeK kt = k;
        kt.elem0 = body; kt.n_elems = E - body;
        const int rc = generic(kt);
        if (rc != HM_OK) return rc;
    }
    return hot_pass();                                     // stream-ordered after the streaming pass: it overwrites the affected elements
}

static int merge_u16_entry(const hm_merge_args* g_in, hm_rules::MergeEntry entry, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16,
                           int bit_depth, void* stream, const double* std_table = nullptr) {
    const hm_rules::U16Extra x{frames_u16, bit_depth, darks_u16, std_table};
    hm_rules::MergeCall call;
    const int rc = hm_rules::check_merge_call(g_in, entry, &x, call);
    if (rc != HM_OK || call.empty) return rc;
    if (g_describe) g_describe->f32 = call.f32out;
    return call.f32out ? merge_u16_launch<OUT_F32>(call, stream) : merge_u16_launch<OUT_F64>(call, stream);
}

// the dispatch above with launching switched off (hm_merge_describe's mechanism). Returns for NULL args before anything else is read - or written.
static int merge_u16_describe(const hm_merge_args* g, hm_rules::MergeEntry entry, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16,
                              int bit_depth, char* buf, int buf_len, const double* std_table = nullptr) {
    if (!buf || buf_len < 1 || !g) return HM_EINVAL;
    DescribeCtx ctx;
    g_describe = &ctx;
    const int rc = merge_u16_entry(g, entry, frames_u16, darks_u16, bit_depth, nullptr, std_table);
    g_describe = nullptr;
    snprintf(buf, static_cast<size_t>(buf_len), "%s", ctx.names.c_str());
    return rc;
}

}  // namespace hm

extern "C" int64_t hm_merge_u16_algorithmic_bytes(const hm_merge_args* g) { return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_U16); }

extern "C" int hm_merge_u16(const hm_merge_args* g, const uint16_t* const* frames_u16, int bit_depth, void* stream) {
    return hm::merge_u16_entry(g, hm_rules::ENTRY_U16, frames_u16, nullptr, bit_depth, stream);
}

extern "C" int hm_merge_u16_describe(const hm_merge_args* g, const uint16_t* const* frames_u16, int bit_depth, char* buf, int buf_len) {
    return hm::merge_u16_describe(g, hm_rules::ENTRY_U16, frames_u16, nullptr, bit_depth, buf, buf_len);
}

// hm_merge_u16 with uint16 dark maps: the same launches, then the hot-pixel pass of hm_merge_u16_hot.hip where a frame has a map
extern "C" int64_t hm_merge_u16_darks_algorithmic_bytes(const hm_merge_args* g, const uint16_t* const* darks_u16) {
    return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_U16_DARKS, darks_u16);
}

extern "C" int hm_merge_u16_darks(const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, int bit_depth, void* stream) {
    return hm::merge_u16_entry(g, hm_rules::ENTRY_U16_DARKS, frames_u16, darks_u16, bit_depth, stream);
}

extern "C" int hm_merge_u16_darks_describe(const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, int bit_depth,
                                           char* buf, int buf_len) {
    return hm::merge_u16_describe(g, hm_rules::ENTRY_U16_DARKS, frames_u16, darks_u16, bit_depth, buf, buf_len);
}

// hm_merge_u16 / hm_merge_u16_darks with the stds from the (2^bit_depth, C) per-DN table: the same dispatch, the LUT instantiations
extern "C" int64_t hm_merge_u16_std_table_algorithmic_bytes(const hm_merge_args* g, const uint16_t* const* darks_u16) {
    return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_U16_STD_TABLE, darks_u16);
}

extern "C" int hm_merge_u16_std_table(const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, const double* std_table,
                                      int bit_depth, void* stream) {
    return hm::merge_u16_entry(g, hm_rules::ENTRY_U16_STD_TABLE, frames_u16, darks_u16, bit_depth, stream, std_table);
}

extern "C" int hm_merge_u16_std_table_describe(const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16,
                                               const double* std_table, int bit_depth, char* buf, int buf_len) {
    return hm::merge_u16_describe(g, hm_rules::ENTRY_U16_STD_TABLE, frames_u16, darks_u16, bit_depth, buf, buf_len, std_table);
}
