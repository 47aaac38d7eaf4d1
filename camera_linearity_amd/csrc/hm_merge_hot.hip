// hm_merge_hot.hip - the one-element-per-thread kernel and the hot-pixel pass of hm_merge_hot.h for float64 std frames (with their val-only
// and per-DN-table forms), and merge_scan_hot, which every form of the pass shares.
#include "hm_merge_hot.h"

namespace hm {

// merge_scan_hot: the scan alone, for 1-byte dark maps (a uint8 DN needs no mask: the literal folds away)
__global__ __launch_bounds__(kScanBlock) void merge_scan_hot(const MergeK a, uint32_t* ws, uint32_t capacity) {
    using D = uint8_t;
    constexpr uint32_t mask = 255u;
#include "hm_merge_hot_scan_body.h"
}

int launch_scan_hot(const MergeK& k, uint32_t* ws, uint32_t capacity, hipStream_t st) {
    const int64_t chunks = (k.n_elems + 15) / 16;
    hipLaunchKernelGGL(merge_scan_hot, dim3(stream_grid(chunks, kScanBlock, 1)), dim3(kScanBlock), 0, st, k, ws, capacity);
    return launch_status();
}

// the instantiations the dispatcher links against (hm_merge_host.h declares them extern)
#define HM_INSTANTIATE_HOT(OUT) \
    template int launch_generic<OUT, double>(const MergeK&, bool, bool, hipStream_t); \
    template int launch_fixup<OUT, double>(const MergeK&, bool, bool, hipStream_t); \
    template int launch_hot_queue<OUT, double>(const MergeK&, bool, bool, uint32_t*, size_t, hipStream_t);
HM_INSTANTIATE_HOT(OUT_F64)
HM_INSTANTIATE_HOT(OUT_F32)
#undef HM_INSTANTIATE_HOT

}  // namespace hm
