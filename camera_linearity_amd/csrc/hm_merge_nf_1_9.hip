// hm_merge_nf_1_9.hip - the compile-time-N merge kernels of hm_merge_nf.h for frame counts 1..9
// (the ranges balance the units' compile times: DESIGN.md 4.1.3).
#include "hm_merge_nf.h"

namespace hm {
HM_INSTANTIATE_NF(1, OUT_F64) HM_INSTANTIATE_NF(2, OUT_F64) HM_INSTANTIATE_NF(3, OUT_F64) HM_INSTANTIATE_NF(4, OUT_F64) HM_INSTANTIATE_NF(5, OUT_F64) HM_INSTANTIATE_NF(6, OUT_F64) HM_INSTANTIATE_NF(7, OUT_F64) HM_INSTANTIATE_NF(8, OUT_F64) HM_INSTANTIATE_NF(9, OUT_F64)
}  // namespace hm
