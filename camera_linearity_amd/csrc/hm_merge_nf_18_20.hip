// hm_merge_nf_18_20.hip - the compile-time-N merge kernels of hm_merge_nf.h for frame counts 18..20
// (the ranges balance the units' compile times: DESIGN.md 4.1.3).
#include "hm_merge_nf.h"

namespace hm {
HM_INSTANTIATE_NF(18, OUT_F64) HM_INSTANTIATE_NF(19, OUT_F64) HM_INSTANTIATE_NF(20, OUT_F64)
}  // namespace hm
