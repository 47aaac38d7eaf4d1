// hm_merge_u16_lut.hip - the per-DN std table's instantiations of the uint16 merge (hm_merge_u16_std_table; gfx950): merge_u16_generic and
// merge_u16_stream with LUT = true, both output types, every table placement. The kernel text is hm_merge_u16_kernels.h, the dispatch and
// the entry points are hm_merge_u16.hip's; a unit of its own so that neither is the build's critical path.
#include "hm_merge_u16_kernels.h"

namespace hm {

#define HM_INSTANTIATE_U16_LUT(OUT) \
    template int launch_u16_generic<OUT, true>(const MergeK&, int, bool, hipStream_t); \
    template int launch_u16_stream<OUT, true>(const MergeK&, int, bool, int, hipStream_t);
HM_INSTANTIATE_U16_LUT(OUT_F64)
HM_INSTANTIATE_U16_LUT(OUT_F32)
#undef HM_INSTANTIATE_U16_LUT

}  // namespace hm
