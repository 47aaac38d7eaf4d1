// hm_pointwise.h - the one kernel of hm_pointwise.hip that another unit launches: k_thresholds behind launch_thresholds()
// (hm_pairs_statistics, hm_stats.hip, thresholds the part of the frames that its LDS loader does not cover).
#pragma once
#include "hm_common.h"

namespace hm {

struct ChanLimits { double lo[HM_MAX_CHANNELS]; double hi[HM_MAX_CHANNELS]; };
// k_thresholds in place on n elements of C <= HM_MAX_CHANNELS channels (sd may be null), with the grid of hm_apply_thresholds
void launch_thresholds(double* val, double* sd, const ChanLimits& lim, int64_t n, int C, hipStream_t st);

}  // namespace hm
