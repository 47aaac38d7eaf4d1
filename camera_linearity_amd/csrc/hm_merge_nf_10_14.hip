// hm_merge_nf_10_14.hip - the compile-time-N merge kernels of hm_merge_nf.h for frame counts 10..14 and the float32 outputs of N = 7
// (the ranges balance the units' compile times: DESIGN.md 4.1.3).
#include "hm_merge_nf.h"

namespace hm {
HM_INSTANTIATE_NF(10, OUT_F64) HM_INSTANTIATE_NF(11, OUT_F64) HM_INSTANTIATE_NF(12, OUT_F64) HM_INSTANTIATE_NF(13, OUT_F64) HM_INSTANTIATE_NF(14, OUT_F64)
HM_INSTANTIATE_NF(7, OUT_F32)
}  // namespace hm
