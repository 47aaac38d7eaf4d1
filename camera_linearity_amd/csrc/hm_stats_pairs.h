// hm_stats_pairs.h - what the all-pairs statistics (hm_stats.hip: hm_pairs_statistics) and the all-pairs distributions (hm_stats_hist.hip:
// hm_pairs_minmax, hm_pairs_histogram) share on the host side: the kernels' argument block and the one fill. Their argument rules are
// hm_pairs_rules.h, shared with the host build. Likewise what the statistics (hm_stats_dn.hip) and the distributions (hm_stats_hist_dn.hip)
// from DN frames share: PairsDnK and the launcher of the table kernel.
#pragma once
#include "hm_common.h"
#include "hm_pairs_rules.h"

namespace hm {

// the frames, pairs (i, j) and multipliers of one launch: a wave (k_pairs_hist: a group of waves) of a workgroup works for one pair
struct PairsK {
    const double* val[HM_MAX_FRAMES];
    const double* sd[HM_MAX_FRAMES];
    int32_t pi[HM_PAIRS_MAX], pj[HM_PAIRS_MAX];
    double mult[HM_PAIRS_MAX];
    int64_t n;
    int32_t C, n_pairs, with_std;
    double lo[HM_MAX_CHANNELS], hi[HM_MAX_CHANNELS];        // apply_thresholds limits per channel (THR instantiations of the LDS kernel)
};

inline void pairs_dist_fill(PairsK& k, const double* const* vals, const double* const* stds, int n_frames, int64_t n, int C,
                            const double* lower, const double* upper) {
    k.n = n; k.C = C; k.with_std = stds ? 1 : 0;
    for (int c = 0; c < HM_MAX_CHANNELS; ++c) {
        k.lo[c] = (lower && c < C) ? lower[c] : -__builtin_huge_val();
        k.hi[c] = (upper && c < C) ? upper[c] : __builtin_huge_val();
    }
    for (int i = 0; i < n_frames; ++i) {
        k.val[i] = vals[i];
        if (stds) k.sd[i] = stds[i];
    }
}

// one workgroup per (pair, difference kind, channel) folds partial[block][pair][channel][kind] of `nblocks` blocks into out (hm_stats.hip)
void launch_pairs_final(const double* partial, int nblocks, int n_pairs, int C, int weighted, double* out, hipStream_t st);

// the DN frames, pairs and multipliers of one launch of the entries that read DN frames (hm_stats_dn.hip, hm_stats_hist_dn.hip)
struct PairsDnK {
    const void* frame[HM_MAX_FRAMES];
    int32_t pi[HM_PAIRS_MAX], pj[HM_PAIRS_MAX];
    double mult[HM_PAIRS_MAX];
    const void* table;                  // entry idx * C + c: {v, s} with stds, v without; thresholds folded in
    int64_t n;
    int32_t C, n_pairs, n_frames;
    uint32_t mask, table_bytes;
};

// k_pairs_dn_table (hm_stats_dn.hip) writes that table - (2^bit_depth, C) entries of 16 bytes with a std_table, 8 without - to `table`
// (16-byte aligned, in the caller's workspace); lower / upper: host, C limits each or both NULL
void launch_pairs_dn_table(const double* icrf, const double* icrf_diff, const double* std_table, const double* lower, const double* upper,
                           int bit_depth, int C, void* table, hipStream_t st);
// ... and fills everything of `k` that does not change from launch to launch
inline void pairs_dn_fill(PairsDnK& k, const void* const* frames, int n_frames, int bit_depth, bool with_std, int64_t n, int C, const void* table) {
    for (int i = 0; i < n_frames; ++i) k.frame[i] = frames[i];
    k.table = table; k.n = n; k.C = C; k.n_frames = n_frames;
    k.mask = (1u << bit_depth) - 1u;
    k.table_bytes = static_cast<uint32_t>(hm_rules::pairs_dn_table_bytes(bit_depth, C, with_std));
}
// the table's place in a workspace: 16-byte aligned at or behind `offset` bytes
inline char* pairs_dn_table_at(void* workspace, size_t offset) {
    char* table = static_cast<char*>(workspace) + offset;
    return table + ((16 - (reinterpret_cast<uintptr_t>(table) & 15u)) & 15u);
}

}  // namespace hm
