// hm_merge_loop.hip - the run-time-N streaming kernels of hm_merge_loop.h for float64 std frames, with their val-only and per-DN-table forms.
#include "hm_merge_loop.h"

namespace hm {
// the instantiations the dispatcher links against (hm_merge_host.h declares them extern)
template int launch_loop<OUT_F64, double>(const MergeK&, bool, hipStream_t);
template int launch_loop<OUT_F32, double>(const MergeK&, bool, hipStream_t);
}  // namespace hm
