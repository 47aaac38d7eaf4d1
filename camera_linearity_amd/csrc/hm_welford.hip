// hm_welford.hip - streaming per-pixel mean / M2 over video frames (gfx950), the producer of the mean and
// STD frames the merge consumes: welford_algorithm, modules/video_processing.py:161-219.
//
//   per frame k (count n = count_before + k + 1):
//       f     = ICRF[dn, c]            (:200-201)      or   dn / 255   (:203)
//       delta = f - mean                                 (:205)
//       mean  = mean + delta / n                         (:206)
//       m2    = m2 + delta * (f - mean)                  (:208)
//   finalize:  mean -> around(mean * 255) as uint8       (:210-211)
//              std  -> around(sqrt(m2 / (n - 1)) / sqrt(n)) as uint8     (:214-215, as written: no * 255)
//
// One launch consumes K frames: the float64 state (16 or 8 B per element) is read and written once per launch
// instead of once per frame, so the traffic per element-frame is 1 + (16 or 32)/K bytes. The frame value comes
// from a 256 x C table in LDS ({dn/255} or the ICRF), two elements per lane (one ushort load per frame, 16-byte
// state accesses: every wave instruction covers whole 128-byte lines).
//
// delta / n carries the bits of NumPy's IEEE division in three dependent FP64 operations inside a range that is checked once per element
// and launch; a lane outside it redoes its elements with the full division (welford_exact). The argument and its predicates:
// hm_welford_dev.h. The lane loop, the fast fold and the finalize loop are the *_body.h texts that hm_welford_u16.hip includes as well.
#include "hm_welford_dev.h"
#include "hm_producer_rules.h"

namespace hm {

struct WelfordK {
    const uint8_t* frame[HM_MAX_FRAMES];
    const double* icrf;          // (256, C) or null
    double* mean;
    double* m2;                  // nullable
    int64_t n;
    int32_t n_frames, C;
    double count0;               // frames already folded into mean / m2
    double rcp[HM_MAX_FRAMES];   // RN(1 / (count0 + k + 1)), formed on the host
};

// The gathers and the exact redo keep their own text beside hm_welford_u16.hip's: every shared form tried moved a kernel.
// reference arithmetic with the IEEE division for `count` consecutive elements, all frames (rare path and odd tail)
template <bool M2>
__device__ __forceinline__ void welford_exact(const WelfordK& a, const double* t, int64_t e0, int count, double* mean, double* m2) {
    for (int j = 0; j < count; ++j) {
        const int64_t e = e0 + j;
        const int c = static_cast<int>(e % a.C);
        double m = a.mean[e], q = M2 ? a.m2[e] : 0.0, cnt = a.count0;
        for (int k = 0; k < a.n_frames; ++k) {
            cnt += 1.0;
            const double f = t[a.frame[k][e] + c * 256];
            const double delta = f - m;                                   // :205
            m = m + delta / cnt;                                          // :206
            if (M2) q = q + delta * (f - m);                              // :208
        }
        mean[j] = m; m2[j] = q;
    }
}

// G frames starting at k0 for the lane's two elements (fast division: the caller has checked its range, hm_welford_dev.h)
template <bool M2, int G, bool VEC>
__device__ __forceinline__ bool welford_group(const WelfordK& a, const double* t, int k0, int64_t e, uint32_t c0, uint32_t c1,
                                              double& cnt, double (&m)[2], double (&q)[2]) {
    uint32_t raw[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        const uint8_t* p = a.frame[k0 + k] + e;
        raw[k] = VEC ? static_cast<uint32_t>(__builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p)))
                     : (p[0] | (static_cast<uint32_t>(p[1]) << 8));
    }
    double f[G][2];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        f[k][0] = t[(raw[k] & 255u) + c0 * 256u];
        f[k][1] = t[(raw[k] >> 8) + c1 * 256u];
    }
#define HM_WELFORD_TEST_GATHERED false
#include "hm_welford_fold_body.h"
}

template <bool M2>
__global__ __launch_bounds__(256) void k_welford(const WelfordK a) {
    __shared__ double t[256 * HM_MAX_CHANNELS];
    const int C = a.C;
    int odd_table = 0;
    for (int i = threadIdx.x; i < 256 * C; i += blockDim.x) {           // t[c][dn]: the gather index is dn + 256 c, no multiply
        const double v = a.icrf ? a.icrf[i] : static_cast<double>(i / C) / 255.0;
        t[(i % C) * 256 + i / C] = v;
        odd_table |= welford_entry_odd(v);
    }
    const bool table_ok = !__syncthreads_or(odd_table);

#define HM_WELFORD_PAIR_ALIGN 2
#define HM_WELFORD_OFFSET(c) (c)
#define HM_WELFORD_GROUP(G, VEC) welford_group<M2, G, VEC>(a, t, k0, e, off0, off1, cnt, m, q)
#define HM_WELFORD_EXACT(e0, count) welford_exact<M2>(a, t, e0, count, m, q)
#include "hm_welford_lane_body.h"
}

__global__ __launch_bounds__(256) void k_welford_finalize(const double* __restrict__ mean, const double* __restrict__ m2,
                                                          double count, uint8_t* __restrict__ out_mean,
                                                          uint8_t* __restrict__ out_std, int64_t n) {
#define HM_WELFORD_SCALE 255.0
#include "hm_welford_finalize_body.h"
}

}  // namespace hm

using namespace hm;

extern "C" int hm_welford_update(const void* const* frames, int n_frames, int64_t count_before, const double* icrf,
                                 double* mean, double* m2, int64_t n_elems, int C, void* stream) {
    bool empty;
    const int rc = hm_rules::check_welford_update(frames, n_frames, count_before, mean, n_elems, C, empty);
    if (rc != HM_OK || empty) return rc;
    WelfordK k{};
    for (int i = 0; i < n_frames; ++i) k.frame[i] = static_cast<const uint8_t*>(frames[i]);
    k.icrf = icrf; k.mean = mean; k.m2 = m2; k.n = n_elems; k.n_frames = n_frames; k.C = C;
    k.count0 = static_cast<double>(count_before);
    for (int i = 0; i < n_frames; ++i) k.rcp[i] = 1.0 / (k.count0 + static_cast<double>(i + 1));
    const unsigned grid = stream_grid((n_elems + 1) / 2, 256, 8);
    if (m2) hipLaunchKernelGGL(k_welford<true>, dim3(grid), dim3(256), 0, as_stream(stream), k);
    else    hipLaunchKernelGGL(k_welford<false>, dim3(grid), dim3(256), 0, as_stream(stream), k);
    return launch_status();
}

extern "C" int hm_welford_finalize(const double* mean, const double* m2, int64_t count, uint8_t* out_mean,
                                   uint8_t* out_std, int64_t n_elems, void* stream) {
    bool empty;
    const int rc = hm_rules::check_welford_finalize(mean, m2, count, out_mean, out_std, n_elems, empty);
    if (rc != HM_OK || empty) return rc;
    const unsigned grid = stream_grid(n_elems, 256, 8);
    hipLaunchKernelGGL(k_welford_finalize, dim3(grid), dim3(256), 0, as_stream(stream), mean, m2,
                       static_cast<double>(count), out_mean, out_std, n_elems);
    return launch_status();
}

extern "C" int64_t hm_welford_algorithmic_bytes(int n_frames, int with_m2, int64_t n_elems) {
    return hm_rules::welford_algorithmic_bytes(1, n_frames, with_m2 != 0, n_elems);
}
