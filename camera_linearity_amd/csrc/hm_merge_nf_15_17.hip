// hm_merge_nf_15_17.hip - the compile-time-N merge kernels of hm_merge_nf.h for frame counts 15..17 and the float32 outputs of N = 15
// (the ranges balance the units' compile times: DESIGN.md 4.1.3).
#include "hm_merge_nf.h"

namespace hm {
HM_INSTANTIATE_NF(15, OUT_F64) HM_INSTANTIATE_NF(16, OUT_F64) HM_INSTANTIATE_NF(17, OUT_F64)
HM_INSTANTIATE_NF(15, OUT_F32)
}  // namespace hm
