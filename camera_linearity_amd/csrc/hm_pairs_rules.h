// hm_pairs_rules.h - the argument rules of the all-pairs entries (hm_pairs_statistics, hm_pairs_minmax, hm_pairs_histogram), written once
// for both builds of the ABI in the manner of hm_merge_rules.h: the device build (hm_stats.hip, hm_stats_hist.hip through hm_stats_pairs.h)
// and the host build (csrc_host/hm_host.cpp) include this file and restate none of it. Plain C++17 on hdrmerge.h: no HIP type.
//
// Every status is here in the order hdrmerge.h gives them: an earlier rule wins over a later one broken in the same call. There is no
// difference between the builds: both ask for the workspace and for 8-byte-aligned frames.
#pragma once
#include "hm_rules_common.h"

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

}  // namespace hm_rules
