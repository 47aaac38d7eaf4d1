// hm_stats_pairs.h - what the all-pairs statistics (hm_stats.hip: hm_pairs_statistics) and the all-pairs distributions (hm_stats_hist.hip:
// hm_pairs_minmax, hm_pairs_histogram) share on the host side: the kernels' argument block, the one argument check and the one fill.
#pragma once
#include "hm_common.h"

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

// the argument checks the three entry points share (hdrmerge.h: the statistics block's codes), in the host build's order
inline int pairs_dist_check(const double* const* vals, const double* const* stds, int n_frames, const int32_t* pair_i, const int32_t* pair_j,
                            const double* multipliers, int n_pairs, int64_t n, int C, const double* lower, const double* upper,
                            const void* out, const void* workspace) {
    if (!vals || !pair_i || !pair_j || !multipliers || !out || !workspace || n < 1 || C < 1 || C > HM_MAX_CHANNELS) return HM_EINVAL;
    if (n_frames < 1 || n_frames > HM_MAX_FRAMES || n_pairs < 1 || ((lower != nullptr) != (upper != nullptr)) || n % C != 0) return HM_EINVAL;
    for (int i = 0; i < n_frames; ++i) if (!vals[i] || (stds && !stds[i])) return HM_EINVAL;
    for (int i = 0; i < n_frames; ++i) if (!aligned(vals[i], 8) || (stds && !aligned(stds[i], 8))) return HM_EALIGN;
    for (int p = 0; p < n_pairs; ++p)
        if (pair_i[p] < 0 || pair_i[p] >= n_frames || pair_j[p] < 0 || pair_j[p] >= n_frames) return HM_EINVAL;
    return HM_OK;
}

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

}  // namespace hm
