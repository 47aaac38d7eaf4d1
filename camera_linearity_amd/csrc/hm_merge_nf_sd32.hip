// hm_merge_nf_sd32.hip - merge_u8_fast_std of hm_merge_nf.h reading float32 std frames (hm_merge_std_f32), for the frame counts of
// kSd32Templated(): N = 7 and N = 15, with and without the flat field, float64 and float32 outputs.
#include "hm_merge_nf.h"

namespace hm {
HM_INSTANTIATE_NF_SD32(7, OUT_F64) HM_INSTANTIATE_NF_SD32(7, OUT_F32)
HM_INSTANTIATE_NF_SD32(15, OUT_F64) HM_INSTANTIATE_NF_SD32(15, OUT_F32)
}  // namespace hm
