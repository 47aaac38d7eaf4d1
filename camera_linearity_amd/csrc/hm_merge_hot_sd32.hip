// hm_merge_hot_sd32.hip - merge_generic, merge_fixup_hot and merge_patch_hot of hm_merge_hot.h reading float32 std frames
// (hm_merge_std_f32): a unit of its own, so the parallel build absorbs it.
#include "hm_merge_hot.h"

namespace hm {
#define HM_INSTANTIATE_HOT(OUT) \
    template int launch_generic<OUT, float>(const MergeK&, bool, bool, hipStream_t); \
    template int launch_fixup<OUT, float>(const MergeK&, bool, bool, hipStream_t); \
    template int launch_hot_queue<OUT, float>(const MergeK&, bool, bool, uint32_t*, size_t, hipStream_t);
HM_INSTANTIATE_HOT(OUT_F64)
HM_INSTANTIATE_HOT(OUT_F32)
#undef HM_INSTANTIATE_HOT
}  // namespace hm
