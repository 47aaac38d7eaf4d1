// hm_pairs_rules.h - the argument rules of the all-pairs entries (hm_pairs_statistics, hm_pairs_minmax, hm_pairs_histogram,
// hm_pairs_statistics_dn, hm_pairs_minmax_dn, hm_pairs_histogram_dn), written once for both builds of the ABI in the manner of
// hm_merge_rules.h: the device build (hm_stats.hip, hm_stats_hist.hip, hm_stats_dn.hip, hm_stats_hist_dn.hip through hm_stats_pairs.h) and
// the host build (csrc_host/hm_host.cpp) include this file and restate none of it. For the DN entries also what both an entry and its
// _describe decide: the table's fit rule, the kernel of a launch, the names.
// Plain C++17 on hdrmerge.h: no HIP type.
//
// Every status is here in the order hdrmerge.h gives them: an earlier rule wins over a later one broken in the same call. There is no
// difference between the builds: both ask for the workspace and for 8-byte-aligned float64 frames (DN frames: check_pairs_dn's own rule).
#pragma once
#include "hm_rules_common.h"
#include <cstdio>

namespace hm_rules {

// the three entries' common arguments; vals, stds (n_frames entries) and pair_i, pair_j (n_pairs entries) are host arrays in both builds
inline int check_pairs(const double* const* vals, const double* const* stds, int n_frames, const int32_t* pair_i, const int32_t* pair_j,
                       const double* multipliers, int n_pairs, int64_t n, int C, const double* lower, const double* upper, const void* out,
                       const void* workspace) {
    if (!vals || !pair_i || !pair_j || !multipliers || !out || !workspace || n < 1 || C < 1 || C > HM_MAX_CHANNELS) return HM_EINVAL;
    if (n_frames < 1 || n_frames > HM_MAX_FRAMES || n_pairs < 1 || ((lower != nullptr) != (upper != nullptr)) || n % C != 0) return HM_EINVAL;
    for (int i = 0; i < n_frames; ++i)
        if (!vals[i] || (stds && !stds[i])) return HM_EINVAL;
    for (int i = 0; i < n_frames; ++i)
        if (!aligned8(vals[i]) || (stds && !aligned8(stds[i]))) return HM_EALIGN;
    for (int p = 0; p < n_pairs; ++p)
        if (pair_i[p] < 0 || pair_i[p] >= n_frames || pair_j[p] < 0 || pair_j[p] >= n_frames) return HM_EINVAL;
    return HM_OK;
}

// hm_pairs_histogram: the common rules, then its own
inline int check_pairs_histogram(const double* const* vals, const double* const* stds, int n_frames, const int32_t* pair_i,
                                 const int32_t* pair_j, const double* multipliers, int n_pairs, int64_t n, int C, int channel_mask,
                                 const double* lower, const double* upper, const double* edges, int bins, const void* out,
                                 const void* workspace) {
    const int rc = check_pairs(vals, stds, n_frames, pair_i, pair_j, multipliers, n_pairs, n, C, lower, upper, out, workspace);
    if (rc != HM_OK) return rc;
    if (bins < 1 || bins > HM_PAIRS_HIST_MAX_BINS || !edges || channel_mask < 0 || (channel_mask >> C) != 0) return HM_EINVAL;
    return HM_OK;
}

// ---- hm_pairs_statistics_dn: the all-pairs statistics straight from uint8 / uint16 DN frames ----
// Everything a frame contributes is a function of (DN & (2^bit_depth - 1), channel): a thresholded {value, std} table entry.
// `variant`: where the staged kernel keeps that table, or the per-wave kernel for every launch.
enum PairsDnVariant { PAIRS_DN_WAVE = -1, PAIRS_DN_AUTO = 0, PAIRS_DN_LDS = 1, PAIRS_DN_GLOBAL = 2 };

constexpr int64_t kPairsDnLdsBytes = 160 * 1024;          // the LDS of a gfx950 CU
constexpr int64_t kPairsDnStagesMax = 3 * 21 * 1024;      // three stages of at most 21 streams, 1 KiB each

// 8 bytes (value) or 16 bytes ({value, std}) per (DN, channel)
inline int64_t pairs_dn_table_bytes(int bit_depth, int C, bool with_std) { return (int64_t{with_std ? 16 : 8} << bit_depth) * C; }
// the fit rule: the table beside the largest stages the staged kernel ever has (a function of the depth, C and the stds alone)
inline bool pairs_dn_table_fits_lds(int bit_depth, int C, bool with_std) {
    return pairs_dn_table_bytes(bit_depth, C, with_std) + kPairsDnStagesMax <= kPairsDnLdsBytes;
}
// frames the staged loader can read an item (two DNs) of with one load: uint8 frames 2-byte, uint16 frames 4-byte aligned
inline bool pairs_dn_frames_item_aligned(const void* const* frames, int n_frames, int bit_depth) {
    const uintptr_t m = bit_depth == 8 ? 1u : 3u;
    for (int i = 0; i < n_frames; ++i)
        if (reinterpret_cast<uintptr_t>(frames[i]) & m) return false;
    return true;
}
// one launch of n_pairs_launch <= HM_PAIRS_MAX pairs: the staged kernel takes it when the frames are item-aligned, a workgroup's threads
// can copy an iteration's 64 * n_frames items with at most two each and the streams fit three stages (hm_pairs_statistics' own rule)
struct PairsDnLaunch { bool staged; int ni; bool tab_lds; };
inline PairsDnLaunch pairs_dn_launch(int n_frames, int n_pairs_launch, bool with_std, int bit_depth, int C, int variant, bool item_aligned) {
    PairsDnLaunch l{};
    const int n_streams = n_frames * (with_std ? 2 : 1);
    l.staged = variant != PAIRS_DN_WAVE && item_aligned && n_frames * 64 <= 2 * 64 * n_pairs_launch && n_streams <= 21;
    l.ni = n_frames * 64 <= 64 * n_pairs_launch ? 1 : 2;
    l.tab_lds = variant == PAIRS_DN_LDS || (variant == PAIRS_DN_AUTO && pairs_dn_table_fits_lds(bit_depth, C, with_std));
    return l;
}

// the rules that look at no pointer: what hm_pairs_statistics_dn_describe checks
inline int check_pairs_dn_counts(int n_frames, int n_pairs, int64_t n, int C, bool with_std, int bit_depth, int variant) {
    if (n < 1 || C < 1 || C > HM_MAX_CHANNELS || n_frames < 1 || n_frames > HM_MAX_FRAMES || n_pairs < 1 || n % C != 0) return HM_EINVAL;
    if (bit_depth < 8 || bit_depth > 16 || variant < PAIRS_DN_WAVE || variant > PAIRS_DN_GLOBAL) return HM_EINVAL;
    if (variant == PAIRS_DN_LDS && !pairs_dn_table_fits_lds(bit_depth, C, with_std)) return HM_EUNSUPPORTED;
    return HM_OK;
}

// What hm_pairs_statistics_dn and the DN distribution entries ask of their common arguments, in hdrmerge.h's order: HM_EINVAL (check_pairs'
// own rules on the frames, bit_depth, a variant outside variant_min..2, std_table without icrf_diff), HM_EALIGN (a table that is not 8-byte
// aligned, a uint16 frame that is not 2-byte aligned), HM_EINVAL for a pair index outside the frames (as check_pairs places it).
inline int check_pairs_dn_args(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff,
                               const double* std_table, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                               int64_t n, int C, const double* lower, const double* upper, int variant, int variant_min, const void* out,
                               const void* workspace) {
    if (!frames || !icrf || !pair_i || !pair_j || !multipliers || !out || !workspace || n < 1 || C < 1 || C > HM_MAX_CHANNELS) return HM_EINVAL;
    if (n_frames < 1 || n_frames > HM_MAX_FRAMES || n_pairs < 1 || ((lower != nullptr) != (upper != nullptr)) || n % C != 0) return HM_EINVAL;
    if (bit_depth < 8 || bit_depth > 16 || variant < variant_min || variant > PAIRS_DN_GLOBAL || (std_table && !icrf_diff)) return HM_EINVAL;
    for (int i = 0; i < n_frames; ++i)
        if (!frames[i]) return HM_EINVAL;
    if (!aligned8(icrf) || !aligned8(icrf_diff) || !aligned8(std_table)) return HM_EALIGN;
    if (bit_depth > 8)
        for (int i = 0; i < n_frames; ++i)
            if (reinterpret_cast<uintptr_t>(frames[i]) & 1u) return HM_EALIGN;
    for (int p = 0; p < n_pairs; ++p)
        if (pair_i[p] < 0 || pair_i[p] >= n_frames || pair_j[p] < 0 || pair_j[p] >= n_frames) return HM_EINVAL;
    return HM_OK;
}

// hm_pairs_statistics_dn: the common rules, then HM_EUNSUPPORTED for variant 1 with a table that does not fit.
inline int check_pairs_dn(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff,
                          const double* std_table, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                          int64_t n, int C, const double* lower, const double* upper, int variant, const void* out, const void* workspace) {
    const int rc = check_pairs_dn_args(frames, n_frames, bit_depth, icrf, icrf_diff, std_table, pair_i, pair_j, multipliers, n_pairs, n, C, lower,
                                       upper, variant, PAIRS_DN_WAVE, out, workspace);
    if (rc != HM_OK) return rc;
    if (variant == PAIRS_DN_LDS && !pairs_dn_table_fits_lds(bit_depth, C, std_table != nullptr)) return HM_EUNSUPPORTED;
    return HM_OK;
}

// the kernels of a call, launch by launch (HM_PAIRS_MAX pairs each), joined by " + ": the device build's names
inline void pairs_dn_describe(int n_frames, int n_pairs, int C, bool with_std, int bit_depth, int variant, bool item_aligned, char* buf,
                              int buf_len) {
    int used = 0;
    buf[0] = '\0';
    for (int p0 = 0; p0 < n_pairs && used < buf_len - 1; p0 += HM_PAIRS_MAX) {
        const int np = n_pairs - p0 < HM_PAIRS_MAX ? n_pairs - p0 : HM_PAIRS_MAX;
        const PairsDnLaunch l = pairs_dn_launch(n_frames, np, with_std, bit_depth, C, variant, item_aligned);
        const char* dn = bit_depth == 8 ? "u8" : "u16";
        int w;
        if (l.staged)
            w = snprintf(buf + used, static_cast<size_t>(buf_len - used), "%spairs_stats_dn_lds<dn=%s,bits=%d,tab=%s,std=%d,ni=%d>", p0 ? " + " : "",
                         dn, bit_depth, l.tab_lds ? "lds" : "global", with_std ? 1 : 0, l.ni);
        else
            w = snprintf(buf + used, static_cast<size_t>(buf_len - used), "%spairs_stats_dn_wave<dn=%s,bits=%d,std=%d>", p0 ? " + " : "", dn,
                         bit_depth, with_std ? 1 : 0);
        if (w < 0 || w >= buf_len - used) break;                                  // (cut short: snprintf has terminated what fitted)
        used += w;
    }
}

// ---- hm_pairs_minmax_dn / hm_pairs_histogram_dn: the all-pairs distributions straight from uint8 / uint16 DN frames ----
// The same thresholded table as above; `variant` 0 / 1 / 2 places it (PAIRS_DN_AUTO / _LDS / _GLOBAL; there is no per-wave form to ask
// for). Here the LDS is what the histograms live in, so the table goes there only where it costs them nothing.
constexpr int kPairsDistBlocks = 252;          // workgroups per CU-share of a distribution grid: a multiple of 12 just below the 256 CUs
constexpr int kPairsDistMaxPerCU = 4;          // workgroups per CU when their LDS and wave count allow it
constexpr int kPairsDistWavesPerCU = 32;       // the waves of 1024-thread workgroups a CU holds

// the min / max partials of a launch of HM_PAIRS_MAX pairs: [grid][pair][kind][HM_MAX_CHANNELS][2] float64
inline int64_t pairs_minmax_partial_bytes() {
    return int64_t{8} * kPairsDistBlocks * kPairsDistMaxPerCU * HM_PAIRS_MAX * 2 * HM_MAX_CHANNELS * 2;
}
// pairs per launch of the histogram kernel with `table_lds_bytes` of the LDS taken by the table (0: the table stays in global memory)
inline int pairs_hist_dn_per_launch(int bins, int C, int64_t table_lds_bytes) {
    const int64_t per_pair = int64_t{2} * C * bins * 8;
    const int64_t fit = (kPairsDnLdsBytes - table_lds_bytes) / per_pair;
    return static_cast<int>(fit > HM_PAIRS_MAX ? HM_PAIRS_MAX : (fit < 0 ? 0 : fit));
}
// launches of equal size: n_pairs at `ppl` per launch at the most (15 pairs at 13 per launch: 8 + 7)
inline int pairs_hist_launches(int n_pairs, int ppl) { return (n_pairs + ppl - 1) / ppl; }
inline int pairs_hist_per(int n_pairs, int ppl) { const int l = pairs_hist_launches(n_pairs, ppl); return (n_pairs + l - 1) / l; }
// waves per pair of a launch of np pairs (fill the workgroup's 16 waves) and the workgroups a CU holds of it: LDS, waves, the cap
inline int pairs_hist_wpp(int np) { return HM_PAIRS_MAX / np; }
inline int pairs_hist_per_cu(int np, int64_t lds_bytes) {
    int per_cu = static_cast<int>(kPairsDnLdsBytes / lds_bytes);
    const int by_waves = kPairsDistWavesPerCU / (np * pairs_hist_wpp(np));
    per_cu = per_cu < by_waves ? per_cu : by_waves;
    per_cu = per_cu < kPairsDistMaxPerCU ? per_cu : kPairsDistMaxPerCU;
    return per_cu < 1 ? 1 : per_cu;
}
// grid of a distribution kernel: `chunk` elements per workgroup and trip, a multiple of 12 workgroups (a lane keeps its channel)
inline int pairs_dist_grid(int64_t n, int per_cu, int chunk) {
    int64_t g = (n + chunk - 1) / chunk;
    g = ((g + 11) / 12) * 12;
    const int64_t cap = static_cast<int64_t>(kPairsDistBlocks) * per_cu;
    return static_cast<int>(g < cap ? g : cap);
}

// The fit rule of hm_pairs_histogram_dn. per: pairs per launch (the last launch may have fewer); ok: false only for variant 1 with a table
// beside which not even one pair's histograms fit. Variant 0 asks for the LDS table call by call - only where the call's pairs take the
// same number of launches with it - and then launch by launch (tab_lds below): only where a CU holds as many workgroups with it.
struct PairsHistDnPlan { bool ok; int per; bool lds_allowed; };
inline PairsHistDnPlan pairs_hist_dn_plan(int n_pairs, int bins, int C, int bit_depth, bool with_std, int variant) {
    const int64_t T = pairs_dn_table_bytes(bit_depth, C, with_std);
    const int ppl0 = pairs_hist_dn_per_launch(bins, C, 0), pplT = pairs_hist_dn_per_launch(bins, C, T);
    if (variant == PAIRS_DN_LDS) return PairsHistDnPlan{pplT >= 1, pplT >= 1 ? pairs_hist_per(n_pairs, pplT) : 0, true};
    const bool same = variant == PAIRS_DN_AUTO && pplT >= 1 && pairs_hist_launches(n_pairs, pplT) == pairs_hist_launches(n_pairs, ppl0);
    return PairsHistDnPlan{true, pairs_hist_per(n_pairs, ppl0), same};
}
// one launch of np pairs of such a call: where its table is
inline bool pairs_hist_dn_tab_lds(const PairsHistDnPlan& plan, int np, int bins, int C, int bit_depth, bool with_std, int variant) {
    if (variant == PAIRS_DN_LDS) return true;
    if (!plan.lds_allowed) return false;
    const int64_t hist = int64_t{2} * C * bins * 8 * np, T = pairs_dn_table_bytes(bit_depth, C, with_std);
    return hist + T <= kPairsDnLdsBytes && pairs_hist_per_cu(np, hist + T) == pairs_hist_per_cu(np, hist);
}
// hm_pairs_minmax_dn holds nothing else in LDS: the table goes there whenever it fits, unless variant 2
inline bool pairs_minmax_dn_tab_lds(int bit_depth, int C, bool with_std, int variant) {
    return variant != PAIRS_DN_GLOBAL && pairs_dn_table_bytes(bit_depth, C, with_std) <= kPairsDnLdsBytes;
}

// hm_pairs_minmax_dn: the common rules (variant 0..2), then HM_EUNSUPPORTED for variant 1 with a table larger than the LDS
inline int check_pairs_minmax_dn(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff,
                                 const double* std_table, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                                 int64_t n, int C, const double* lower, const double* upper, int variant, const void* out,
                                 const void* workspace) {
    const int rc = check_pairs_dn_args(frames, n_frames, bit_depth, icrf, icrf_diff, std_table, pair_i, pair_j, multipliers, n_pairs, n, C, lower,
                                       upper, variant, PAIRS_DN_AUTO, out, workspace);
    if (rc != HM_OK) return rc;
    if (variant == PAIRS_DN_LDS && !pairs_minmax_dn_tab_lds(bit_depth, C, std_table != nullptr, variant)) return HM_EUNSUPPORTED;
    return HM_OK;
}
// hm_pairs_histogram_dn: the common rules, hm_pairs_histogram's own where check_pairs_histogram has them, then the fit rule
inline int check_pairs_histogram_dn(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff,
                                    const double* std_table, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers,
                                    int n_pairs, int64_t n, int C, int channel_mask, const double* lower, const double* upper,
                                    const double* edges, int bins, int variant, const void* out, const void* workspace) {
    const int rc = check_pairs_dn_args(frames, n_frames, bit_depth, icrf, icrf_diff, std_table, pair_i, pair_j, multipliers, n_pairs, n, C, lower,
                                       upper, variant, PAIRS_DN_AUTO, out, workspace);
    if (rc != HM_OK) return rc;
    if (bins < 1 || bins > HM_PAIRS_HIST_MAX_BINS || !edges || channel_mask < 0 || (channel_mask >> C) != 0) return HM_EINVAL;
    if (!pairs_hist_dn_plan(n_pairs, bins, C, bit_depth, std_table != nullptr, variant).ok) return HM_EUNSUPPORTED;
    return HM_OK;
}
// the rules that look at no pointer: what hm_pairs_histogram_dn_describe checks
inline int check_pairs_hist_dn_counts(int n_frames, int n_pairs, int64_t n, int C, bool with_std, int bit_depth, int bins, int variant) {
    if (n < 1 || C < 1 || C > HM_MAX_CHANNELS || n_frames < 1 || n_frames > HM_MAX_FRAMES || n_pairs < 1 || n % C != 0) return HM_EINVAL;
    if (bit_depth < 8 || bit_depth > 16 || variant < PAIRS_DN_AUTO || variant > PAIRS_DN_GLOBAL) return HM_EINVAL;
    if (bins < 1 || bins > HM_PAIRS_HIST_MAX_BINS) return HM_EINVAL;
    if (!pairs_hist_dn_plan(n_pairs, bins, C, bit_depth, with_std, variant).ok) return HM_EUNSUPPORTED;
    return HM_OK;
}

// the histogram kernel of every launch of a call, joined by " + ": the device build's names
inline void pairs_hist_dn_describe(int n_pairs, int C, bool with_std, int bit_depth, int bins, int variant, char* buf, int buf_len) {
    const PairsHistDnPlan plan = pairs_hist_dn_plan(n_pairs, bins, C, bit_depth, with_std, variant);
    int used = 0;
    buf[0] = '\0';
    for (int p0 = 0; p0 < n_pairs && used < buf_len - 1; p0 += plan.per) {
        const int np = n_pairs - p0 < plan.per ? n_pairs - p0 : plan.per;
        const bool lds = pairs_hist_dn_tab_lds(plan, np, bins, C, bit_depth, with_std, variant);
        const int w = snprintf(buf + used, static_cast<size_t>(buf_len - used), "%spairs_hist_dn<dn=%s,bits=%d,tab=%s,std=%d,np=%d,wpp=%d>",
                               p0 ? " + " : "", bit_depth == 8 ? "u8" : "u16", bit_depth, lds ? "lds" : "global", with_std ? 1 : 0, np,
                               pairs_hist_wpp(np));
        if (w < 0 || w >= buf_len - used) break;                                  // (cut short: snprintf has terminated what fitted)
        used += w;
    }
}

}  // namespace hm_rules
