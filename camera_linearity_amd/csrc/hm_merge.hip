// hm_merge.hip - fused HDR merge for gfx950 (MI355X).
//
// Replaces, in one call, the two passes of the reference's merge loop
// (modules/exposure_series.py:317-345 `_precalculate_sum_of_weights` and :347-397
// `_compute_HDR_image_set`) together with the per-frame arithmetic they call:
// apply_gaussian_weight (modules/measurand.py:606-618), linearize (:471-541), the optional hot-pixel
// median (:543-557) and the optional flat-field normalisation (:559-604).
//
// The path is HBM-bandwidth bound (no MFMA): every input byte is read once with coalesced loads, every
// output byte written once. Per (element, frame) the only arithmetic is a table gather, because for
// 8-bit frames both the Gaussian weight and the ICRF depend on the DN alone; the 256-entry tables
// (w, w*g per channel, ...) live in LDS.
//
// Kernels (hm_merge dispatches; all share one operation sequence per output element, so a result does not depend on
// which kernel or tiling produced it) and the file each family lives in:
//   merge_u8_val3                       uint8 frames, C == 3, N <= 20 (compile-time), val-only, no extras: the bench kernel (config 2).
//   merge_u8_fast / merge_u8_fast_std   the same frames with std, flat field or sum-of-weights output (config 3).
//                     hm_merge_nf.h (with merge_u8_fast_std_lut, the per-DN std table's form), instantiated per range of frame
//                     counts by hm_merge_nf_*.hip.
//   merge_u8_loop / merge_u8_loop_std   uint8 frames, run-time N (17..32) and C (1..4): same decomposition, frames in chunks.
//                     hm_merge_loop.h, instantiated by hm_merge_loop.hip (and hm_merge_loop_sd32.hip)
//   merge_f64_val / merge_f64_std       float64 frames (64-bit mode): analytic weight, computed LUT index.
//                     hm_merge_f64.hip
//   merge_generic     anything else (tails shorter than a group, unaligned tiles, forced by variant < 0):
//                     one element per thread. hm_merge_hot.h (instantiated by hm_merge_hot.hip and hm_merge_hot_sd32.hip), with the hot-pixel kernels:
//   merge_scan_hot + merge_patch_hot    dark-frame hot pixels: the streaming kernels never look at the dark maps; a scan reads every
//                     distinct map once (the d term of the algorithmic byte count) and queues the hot elements, a second kernel
//                     recomputes one queued element per lane with the k x k medians substituted (needs the caller's workspace).
//   merge_fixup_hot   the same pass without a workspace: one hot element per wave at a time (sparse maps only).
// Every kernel that stores val / std has a template parameter OUT (hm_merge_args.out_kind): OUT_F64 stores the float64 result,
// OUT_F32 rounds it once in registers (v_cvt_f32_f64, round to nearest even) and stores 4-byte elements. Nothing else differs.
// Every kernel that reads std frames has a template parameter SD (hm_merge_std_f32): SD = float reads 4-byte std elements and widens each
// once in registers (exact), so the result equals that of the widened frames bit for bit. Its instantiations live in units of their own
// (hm_merge_nf_sd32.hip, hm_merge_loop_sd32.hip, hm_merge_hot_sd32.hip).
//
// This file is the host side of the call: the dispatch (merge_entry, merge_one_launch) and the C entry points.
// It holds no kernel and instantiates none: hm_merge_dev.h has what the families share on the device, hm_merge_host.h the describe
// context, the launch geometry and the family launchers' declarations. Stacks of more than HM_MAX_FRAMES frames: hm_merge_chunk.hip.
// The argument rules of the three entry points (accepted layouts, the order of the checks, the algorithmic byte count) are not here:
// hm_merge_rules.h has the one copy that this build and the host build (csrc_host/hm_host.cpp) both compile; merge_entry adds the two
// refusals that are this build's own.
#include "hm_merge_host.h"
#include "hm_merge_rules.h"

namespace hm {

thread_local DescribeCtx* g_describe = nullptr;
bool describe_only(const char* fmt, int a, int b, int c, int d, bool quad) {
    if (!g_describe) return false;
    char buf[160];
    snprintf(buf, sizeof buf, fmt, a, b, c, d);
    std::string name = buf;
    // float32 calls: every kernel that stores val / std (all of them have a template argument list) says so inside it;
    // the strings of float64 calls stay as they were
    // table calls: likewise every kernel that forms a std (in such a call: every kernel with a template argument list) carries "std=lut"
    size_t close = name.find('>');
    // float32-std calls (hm_merge_std_f32): likewise "std=f32" - merge_scan_hot, which reads no std, has no argument list
    if (g_describe->lut && close != std::string::npos) { name.insert(close, ",std=lut"); close = name.find('>'); }
    if (g_describe->sd32 && close != std::string::npos) { name.insert(close, ",std=f32"); close = name.find('>'); }
    if (g_describe->f32 && close != std::string::npos) name.insert(close, quad ? ",out=f32x4" : ",out=f32");
    if (!g_describe->names.empty()) g_describe->names += " + ";
    g_describe->names += name;
    return true;
}

static bool decode_variant(int variant, bool with_std, FastCfg& c) {
    c = default_cfg(with_std);
    if (variant <= 0) return true;
    const int tab = variant / 1000, pf = (variant / 100) % 10, u = (variant / 10) % 10, bc = variant % 10;
    if (with_std) {                                   // std kernel: only U (1, 2, 4) and PREFETCH are tunable
        if (pf > 1 || (u != 1 && u != 2 && u != 4)) return false;
        c.u = u; c.prefetch = pf;
        return true;
    }
#ifndef HM_PROBE
    if (tab == TAB_NONE) return false;                // the table-free traffic probe (wrong results) exists in -DHM_PROBE builds only
#endif
    if ((tab != TAB_PLAIN && tab != TAB_FUSED && tab != TAB_NONE) || pf > 1 || (u != 2 && u != 4 && u != 8) || bc > 1) return false;
    c.tab = tab; c.u = u; c.prefetch = pf; c.block = bc ? 1024 : 256;
    return true;
}

// elements per group of the configuration launch_fast_nf() will really use
static int fast_group_elems(int n_frames, int variant, const FastCfg& c, bool with_std, bool extras, bool val3_flat) {
    if (val3_flat) return val3_unit_elems(val3_flat_default(n_frames));
    { int pu = 0; if (!with_std && !extras && priv_variant(variant, n_frames, pu)) return pu * 120; }     // merge_u8_priv's chunks (tuning builds)
    { Val3Cfg vc; if (!with_std && !extras && val3_variant(variant, n_frames, vc)) return val3_unit_elems(vc); }
    if (with_std) return ((extras || n_frames != HM_TUNE_NF) ? kUStd : c.u) * static_cast<int>(kSub);
    if (extras || n_frames != HM_TUNE_NF) return kUVal * static_cast<int>(kSub);
    return c.u * static_cast<int>(kSub);
}

}  // namespace hm

using hm_rules::MergeCall;
using hm_rules::MergeEntry;

extern "C" int64_t hm_merge_algorithmic_bytes(const hm_merge_args* g) { return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_MERGE); }
extern "C" int64_t hm_merge_std_table_algorithmic_bytes(const hm_merge_args* g) { return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_STD_TABLE); }
extern "C" int64_t hm_merge_std_f32_algorithmic_bytes(const hm_merge_args* g) { return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_STD_F32); }

// Workspace of the hot-pixel queue for a call that produces n_elems = rows * W * C output elements: 16 bytes of counters, the piece
// table (8 bytes per 65 536 elements + 8 KB) and one uint32 per queued element. The recommended size holds a quarter of the elements
// (a dark map with 25 % hot pixels); a workspace with room for at least one entry (hm_merge_hot_workspace_min_bytes) is accepted - a
// queue that overflows makes the patch kernel go over the whole tile; a smaller one selects the workspace-free pass.
extern "C" size_t hm_merge_hot_workspace_min_bytes(int64_t n_elems) {
    if (n_elems < 1) n_elems = 1;
    return (static_cast<size_t>(hm::kHotQueueHeader) + 2u * hm::hot_piece_slots(n_elems) + 1u) * 4;
}
extern "C" size_t hm_merge_hot_workspace_bytes(int64_t n_elems) {
    if (n_elems < 1) n_elems = 1;
    int64_t entries = n_elems / 4;
    if (entries < 4096) entries = n_elems < 4096 ? n_elems : 4096;
    return hm_merge_hot_workspace_min_bytes(n_elems) + static_cast<size_t>(entries - 1) * 4;
}

static int merge_entry(const hm_merge_args* g_in, MergeEntry entry, const void* extra, void* stream);

// extra: the entry's own pointer (hm_merge_rules.h). The std entries return for NULL args before anything else is read - or written.
static int merge_describe(const hm_merge_args* g, MergeEntry entry, const void* extra, char* buf, int buf_len) {
    if (!buf || buf_len < 1 || (!g && entry != hm_rules::ENTRY_MERGE)) return HM_EINVAL;
    hm::DescribeCtx ctx;                                   // f32 / lut / sd32: set by merge_entry once it has accepted such a call
    hm::g_describe = &ctx;
    const int rc = merge_entry(g, entry, extra, nullptr);
    hm::g_describe = nullptr;
    snprintf(buf, static_cast<size_t>(buf_len), "%s", ctx.names.c_str());
    return rc;
}
extern "C" int hm_merge_describe(const hm_merge_args* g, char* buf, int buf_len) { return merge_describe(g, hm_rules::ENTRY_MERGE, nullptr, buf, buf_len); }
extern "C" int hm_merge_std_table_describe(const hm_merge_args* g, const double* std_table, char* buf, int buf_len) {
    return merge_describe(g, hm_rules::ENTRY_STD_TABLE, std_table, buf, buf_len);
}
extern "C" int hm_merge_std_f32_describe(const hm_merge_args* g, const float* const* stds_f32, char* buf, int buf_len) {
    return merge_describe(g, hm_rules::ENTRY_STD_F32, stds_f32, buf, buf_len);
}

extern "C" int hm_merge(const hm_merge_args* g, void* stream) { return merge_entry(g, hm_rules::ENTRY_MERGE, nullptr, stream); }
// hm_merge's path with the table / the float32 frames in the place of the std frames
extern "C" int hm_merge_std_table(const hm_merge_args* g, const double* std_table, void* stream) { return merge_entry(g, hm_rules::ENTRY_STD_TABLE, std_table, stream); }
extern "C" int hm_merge_std_f32(const hm_merge_args* g, const float* const* stds_f32, void* stream) { return merge_entry(g, hm_rules::ENTRY_STD_F32, stds_f32, stream); }

template <int OUT>
static int merge_one_launch(const MergeCall& call, void* stream);
static int merge_launch(const MergeCall& call, void* stream) {
    return call.f32out ? merge_one_launch<hm::OUT_F32>(call, stream) : merge_one_launch<hm::OUT_F64>(call, stream);
}

// The argument rules of all three entries are hm_merge_rules.h's (shared with the host build); this build adds two refusals of its own.
static int merge_entry(const hm_merge_args* g_in, MergeEntry entry, const void* extra, void* stream) {
    using namespace hm;
    MergeCall call;
    const int rc_args = hm_rules::check_merge_call(g_in, entry, extra, call);
    if (rc_args != HM_OK || call.empty) return rc_args;
    const hm_merge_args* g = &call.a;
    const int N = g->n_frames, C = g->channels;
    // the per-DN std table exists in the one-launch kernels only (hm_merge_chunk.hip reads std frames)
    if (call.std_src == hm_rules::STD_TABLE && (N > HM_MAX_FRAMES || g->variant <= -2)) return HM_EUNSUPPORTED;
    // the variant matrix of a tuning build is float64 instantiations
    if (call.f32out && HM_TUNE_NF != 0 && g->variant > 0) return HM_EUNSUPPORTED;
    if (g_describe) { g_describe->f32 = call.f32out; g_describe->lut = call.std_src == hm_rules::STD_TABLE; g_describe->sd32 = call.std_src == hm_rules::STD_F32; }
    // More frames than one launch takes (modules/exposure_series.py:334,372 have no limit): HM_MAX_FRAMES per launch with the running
    // sums in memory (hm_merge_chunk.hip). variant <= -2 forces that path with -variant frames per chunk (tests: any chunking gives the
    // bits of the one-launch kernels).
    if (N > HM_MAX_FRAMES || g->variant <= -2) {
        int chunk = g->variant <= -2 ? -g->variant : HM_MAX_FRAMES;
        if (chunk > HM_MAX_FRAMES) chunk = HM_MAX_FRAMES;
        return merge_chunked(g, chunk, g_describe ? &g_describe->names : nullptr, as_stream(stream));
    }
    // The streaming kernels index groups and buffer offsets with 32 bits: a tile of 2^32 elements or more is merged as consecutive
    // row bands of fewer than 2^32 elements each (same buffers, row0 / rows / output pointers advanced; an even number of rows per band
    // keeps every band's first byte 2-byte aligned). Only a single row of >= 2^32 elements is left to merge_generic.
    {
        const int64_t per_row = g->width * static_cast<int64_t>(C);
        const int64_t limit = (int64_t{1} << 32) - 1;
        if (g->rows * per_row > limit && per_row <= limit / 2 && g->variant >= 0) {
            int64_t band_rows = limit / per_row;
            if (band_rows > 1) band_rows &= ~int64_t{1};
            for (int64_t r = 0; r < g->rows; r += band_rows) {
                MergeCall band = call;                                 // (a band of a valid tile is valid: the rules are not asked again)
                hm_merge_args& b = band.a;
                b.row0 = g->row0 + r;
                b.rows = g->rows - r < band_rows ? g->rows - r : band_rows;
                const int64_t adv = r * per_row;                       // outputs and the flat field cover the OUTPUT rows
                if (g->out_val) b.out_val = g->out_val + adv;
                if (g->out_std) b.out_std = g->out_std + adv;
                if (g->out_sum_w) b.out_sum_w = g->out_sum_w + adv;
                if (g->flat_u8) b.flat_u8 = g->flat_u8 + adv;
                if (g->flat_f64) b.flat_f64 = g->flat_f64 + adv;
                if (g->flat_std) b.flat_std = g->flat_std + adv;
                const int rc_b = merge_launch(band, stream);
                if (rc_b != HM_OK) return rc_b;
            }
            return HM_OK;
        }
    }
    return merge_launch(call, stream);
}

// One streaming launch (+ generic tail + hot-pixel pass) for validated arguments; OUT = element type of out_val / out_std.
template <int OUT>
static int merge_one_launch(const MergeCall& call, void* stream) {
    using namespace hm;
    const hm_merge_args* g = &call.a;
    const double* const std_table = call.std_table;
    const bool sd32 = call.std_src == hm_rules::STD_F32, f64in = call.f64in, with_std = call.with_std, flat = call.flat, hot = call.hot;
    const int N = g->n_frames, C = g->channels;
    const bool f32_pairs = OUT == OUT_F32 && g->variant == kVariantF32Pairs;      // float32 A/B: the default dispatch without the QUAD map
    const int variant = f32_pairs ? 0 : g->variant;
    MergeK k{};
    for (int i = 0; i < N; ++i) {
        k.frame[i] = f64in ? static_cast<const void*>(g->frames_f64[i]) : static_cast<const void*>(g->frames_u8[i]);
        if (g->stds) k.sd[i] = g->stds[i];
        k.inv_t[i] = 1.0 / g->exposures[i];
        k.dark[i] = hot ? g->darks_u8[i] : nullptr;
        k.dark_min[i] = hot && g->dark_min_dn ? g->dark_min_dn[i] : 256;
    }
    k.icrf = g->icrf; k.icrf_diff = g->icrf_diff; k.w_lut = g->w_lut; k.dw_lut = g->dw_lut; k.std_lut = std_table;
    k.flat_u8 = g->flat_u8; k.flat_f64 = g->flat_f64; k.flat_std = g->flat_std;
    for (int c = 0; c < HM_MAX_CHANNELS; ++c) { k.ff_mean[c] = g->ff_mean[c]; k.ff_std_mean[c] = g->ff_std_mean[c]; }
    k.out_val = g->out_val; k.out_std = g->out_std; k.out_sum_w = g->out_sum_w;
    const int64_t E = g->rows * g->width * C;
    k.n_elems = E; k.elem0 = 0;
    k.in_off = (g->row0 - g->buf_row0) * g->width * C;
    k.H = g->height; k.W = g->width; k.row0 = g->row0; k.buf_row0 = g->buf_row0; k.buf_rows = g->buf_rows;
    k.n_frames = N; k.C = C; k.median_k = hot ? g->median_k : 3; k.has_flat = flat ? 1 : 0;
    k.variant = variant;
    k.inv_t_inrange = 1;
    for (int i = 0; i < N; ++i) k.inv_t_inrange = k.inv_t_inrange && k.inv_t[i] >= 0x1p-300 && k.inv_t[i] <= 0x1p300;
    hipStream_t st = as_stream(stream);
    const bool hot_queue = hot && g->hot_workspace && g->hot_workspace_bytes >= hm_merge_hot_workspace_min_bytes(g->rows * g->width * C) &&
                           aligned(g->hot_workspace, 16) && g->rows * g->width * C < (int64_t{1} << 32);
    k.hot_reset = hot_queue ? static_cast<uint32_t*>(g->hot_workspace) : nullptr;

    // ---- streaming pass: fast kernel where eligible, generic kernel otherwise (dark maps are not read here)
    FastCfg cfg;
    const int tune_variant = (HM_TUNE_NF != 0 && variant >= 10000) ? variant % 10000 : variant;   // W * 10000 + 7UPM (tuning builds)
    if (tune_variant >= 7000 && tune_variant < 9000) {        // merge_u8_val3 / merge_u8_priv A/B variants (tuning builds)
        Val3Cfg vc;
        int pu = 0;
        const bool ok = tune_variant < 8000 ? val3_variant(variant, N, vc) : priv_variant(variant, N, pu);
        if (!ok || with_std || flat || g->out_sum_w || f64in || C != 3) return HM_EINVAL;
        cfg = default_cfg(with_std);
    } else if (!decode_variant(variant, with_std, cfg)) return HM_EINVAL;
    // (the per-DN std table: uint8 frames stream through the kernels that hold it in LDS; float64 frames go to merge_generic - merge_f64_std reads std frames)
    const bool lut = std_table != nullptr;
    // (float32 std frames likewise: uint8 frames stream, float64 frames go to merge_generic)
    bool fast = g->out_val && E < (int64_t{1} << 32) && variant >= 0 && !((lut || sd32) && f64in);
    // (float32 outputs: templated kernels for the frame counts of kF32Templated() only - build time; the others take the run-time-N kernels)
    const bool templated = OUT == OUT_F64 || kF32Templated(N);
    const bool mono_val3 = templated && use_val3_mono(k, with_std, f64in);
    const bool mono_std = templated && !lut && use_fast_std_mono(k, with_std, f64in);
    const bool lut_templated = OUT == OUT_F64 && use_fast_lut(k, f64in);
    // Templates up to kTemplatedN = 20 frames (round 4, late: 16 before). On 2048 x 4096 x 3 stacks the templated kernels beat the run-time-N
    // kernel at N = 17 (val-only 115 against 130 us, with std 790 against 880 us) and N = 20 (132 against 150, 985 against 1 025 us) and lose from
    // N = 24 (with std) / 32 (val-only) on, where their per-frame register arrays no longer fit (profiles/r04z_n32_templates_ab.log).
    const bool sd32_templated = use_fast_sd32(k, sd32, f64in);
    const bool loop_kernel = lut ? !lut_templated : sd32 ? !sd32_templated
                                 : (f64in || N > kTemplatedN || C != 3 || !templated) && !mono_val3 && !mono_std;   // run-time-N / any-C streaming kernel instead of the templates
    if (fast) {
        for (int i = 0; i < N && fast; ++i) {
            fast = f64in ? aligned(static_cast<const double*>(k.frame[i]) + k.in_off, 16)
                         : aligned(static_cast<const uint8_t*>(k.frame[i]) + k.in_off, 2);
            // (float32 stds: the lane's pair is one 8-byte load - the first element at an even offset, every std buffer 8-byte aligned there)
            if (fast && with_std && !lut) fast = sd32 ? (k.in_off % 2 == 0 && aligned(k.sd_as<float>(i) + k.in_off, 8)) : aligned(k.sd[i] + k.in_off, 16);
        }
        constexpr int pair_bytes = OUT == OUT_F32 ? 8 : 16;                  // one lane's two output elements
        fast = fast && aligned(k.out_val, pair_bytes) && (!k.out_std || aligned(k.out_std, pair_bytes)) &&
               (!k.out_sum_w || aligned(k.out_sum_w, 16));
        if (fast && flat)
            fast = (k.flat_u8 ? aligned(k.flat_u8, 2) : aligned(k.flat_f64, 16)) && (!with_std || aligned(k.flat_std, 16));
    }
    // the families with a std element type: SD = float for hm_merge_std_f32
    const auto generic = [&](const MergeK& kk) { return sd32 ? launch_generic<OUT, float>(kk, f64in, with_std, st) : launch_generic<OUT>(kk, f64in, with_std, st); };
    const auto loop = [&](const MergeK& kk) { return sd32 ? launch_loop<OUT, float>(kk, with_std, st) : launch_loop<OUT>(kk, with_std, st); };
    int rc = HM_OK;
    if (!fast) {
        rc = generic(k);
    } else {
        const int64_t grp = loop_kernel ? static_cast<int64_t>(kSub) : lut_templated ? static_cast<int64_t>(HM_LUT_U) * kSub : (mono_val3 ? val3_unit_elems(flat ? val3_flat_default(N) : val3_default(N))
                                                                                                 : fast_group_elems(N, variant, cfg, with_std, flat || g->out_sum_w, use_val3_flat(k, with_std)));
        const int64_t body = (E / grp) * grp;
        if (body > 0) {
            MergeK kb = k;
            kb.n_elems = body;
            if (sd32_templated) {
                switch (N) {
                    case 7: rc = launch_fast_nf_sd32<7, OUT>(kb, st); break;
                    case 15: rc = launch_fast_nf_sd32<15, OUT>(kb, st); break;
                    static_assert(kSd32Templated(7) && kSd32Templated(15) && !kSd32Templated(8), "one case per float32-std-templated frame count");
                    default: rc = HM_EINVAL; break;
                }
            } else if constexpr (OUT == OUT_F32) {
                switch (loop_kernel ? 0 : N) {
                    case 7: rc = launch_fast_nf<7, OUT_F32>(kb, cfg, with_std, !f32_pairs, st); break;
                    case 15: rc = launch_fast_nf<15, OUT_F32>(kb, cfg, with_std, !f32_pairs, st); break;
                    static_assert(kF32Templated(7) && kF32Templated(15) && !kF32Templated(8), "one case per float32-templated frame count");
                    default: rc = f64in ? launch_f64<OUT>(kb, with_std, st) : loop(kb); break;
                }
            } else {
            switch (loop_kernel ? 0 : N) {
#define HM_CASE(n) case n: rc = launch_fast_nf<n, OUT_F64>(kb, cfg, with_std, false, st); break;
                HM_CASE(1) HM_CASE(2) HM_CASE(3) HM_CASE(4) HM_CASE(5) HM_CASE(6) HM_CASE(7) HM_CASE(8)
                HM_CASE(9) HM_CASE(10) HM_CASE(11) HM_CASE(12) HM_CASE(13) HM_CASE(14) HM_CASE(15) HM_CASE(16)
                HM_CASE(17) HM_CASE(18) HM_CASE(19) HM_CASE(20)
                static_assert(kTemplatedN == 20, "one HM_CASE per templated frame count");
#undef HM_CASE
                default: rc = f64in ? launch_f64<OUT>(kb, with_std, st) : loop(kb); break;   // run-time frame count
            }
            }
            if (rc != HM_OK) return rc;
        }
        if (body < E) {                                    // tail: less than one group
            MergeK kt = k;
            kt.elem0 = body; kt.n_elems = E - body;
            rc = generic(kt);
        }
    }
    if (rc != HM_OK) return rc;
    // ---- hot-pixel fix-up pass (stream-ordered after the streaming pass: it overwrites the affected elements)
    if (hot) {
        if (sd32) rc = hot_queue ? launch_hot_queue<OUT, float>(k, f64in, with_std, static_cast<uint32_t*>(g->hot_workspace), g->hot_workspace_bytes, st)
                             : launch_fixup<OUT, float>(k, f64in, with_std, st);
        else rc = hot_queue ? launch_hot_queue<OUT>(k, f64in, with_std, static_cast<uint32_t*>(g->hot_workspace), g->hot_workspace_bytes, st)
                   : launch_fixup<OUT>(k, f64in, with_std, st);
    }
    return rc;
}
