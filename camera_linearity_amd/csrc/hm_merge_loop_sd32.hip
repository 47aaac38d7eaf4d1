// hm_merge_loop_sd32.hip - merge_u8_loop_std of hm_merge_loop.h reading float32 std frames (hm_merge_std_f32): a unit of its own, so the
// parallel build absorbs its sixteen kernels.
#include "hm_merge_loop.h"

namespace hm {
template int launch_loop<OUT_F64, float>(const MergeK&, bool, hipStream_t);
template int launch_loop<OUT_F32, float>(const MergeK&, bool, hipStream_t);
}  // namespace hm
