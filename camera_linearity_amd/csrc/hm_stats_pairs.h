// hm_stats_pairs.h - what the all-pairs statistics (hm_stats.hip: hm_pairs_statistics) and the all-pairs distributions (hm_stats_hist.hip:
// hm_pairs_minmax, hm_pairs_histogram) share on the host side: the kernels' argument block and the one fill. Their argument rules are
// hm_pairs_rules.h, shared with the host build.
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

}  // namespace hm
