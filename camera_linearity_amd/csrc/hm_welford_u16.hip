// hm_welford_u16.hip - hm_welford.hip's streaming per-pixel mean / M2 for 9- to 16-bit cameras (gfx950): uint16 HWC frames with an explicit
// bit depth b, M = 2^b - 1 (hdrmerge.h: hm_welford_update_u16, hm_welford_finalize_u16). The arithmetic and its references are described
// in hm_welford.hip; this unit keeps that kernel's decomposition - the lane loop is the same text, hm_welford_lane_body.h - and changes
// only where a frame value comes from:
//
//   per frame k (count n = count_before + k + 1):
//       f     = ICRF[DN & M, c]     or   (DN & M) / M
//       delta = f - mean;   mean = mean + delta / n;   m2 = m2 + delta * (f - mean)
//   finalize:  mean -> around(mean * M) as uint16;   std -> around(sqrt(m2 / (n - 1)) / sqrt(n)) as uint16   (as written: no * M)
//
// k_welford_u16<M2, PLACE>: k_welford's lane loop with one 4-byte load per frame (two uint16 DNs). The pair rule: frames 4-byte aligned at
// the first element and state 16-byte aligned; a call that breaks it takes the scalar loads and stores with the same bits. DN & M is
// applied before every table access, in LDS or global memory.
//
// PLACE (hm_rules::WelfordU16Tab; the fit rule and the default are hm_producer_rules.h's) says where f comes from:
//   tab=lds       dynamic LDS: the ICRF as t[ch][dn] (8 * 2^b * C bytes), or without an ICRF the one column dn / M (8 * 2^b bytes, formed
//                 with the IEEE division while the table is filled). One workgroup of 1024 threads per CU, as merge_u16_stream; the
//                 dynamic-LDS maximum of these instantiations is raised once per process by a host-side call that enqueues nothing.
//                 The first 16 bytes of the region hold the workgroup's "odd table" word; there is no static LDS (the table stays 16-byte
//                 aligned).
//   tab=computed  no ICRF only: f = dn / M in three dependent FP64 operations with r = RN(1 / M) from the host,
//                     q0 = dn * r;   e = fma(-q0, M, dn);   f = fma(e, r, q0)
//                 which is the IEEE quotient for every dn of every depth 9..16 (130 560 cases, checked with exact rational arithmetic and
//                 again through the library by tests/test_welford_u16_host.py::check_computed_quotient).
//   tab=global    the ICRF gathered from global memory at icrf[dn * C + c]; 256-thread workgroups.
//
// The fast-division range argument of hm_welford_dev.h (every non-zero delta >= 2^-900 when table entries are 0 or in
// [2^-500, 2^500], the incoming mean is 0 or in [2^-540, 2^500], |m2| <= 2^900 and n <= 2^40) holds in every placement because each one
// establishes the table condition before a fast result is kept; the state is checked at load in all of them:
//   tab=lds       every entry is tested while the table is filled; one odd entry sends the whole workgroup to welford_exact.
//   tab=computed  f is 0 or in [1 / 65535, 1]: nothing to test.
//   tab=global    nobody has seen the whole table, so a lane tests every value it gathers (the compares sit under the gathers' latency)
//                 and redoes its two elements with welford_exact if one of them is outside the range. A fast result is kept only when
//                 every f that went into it was inside, which is all the argument needs: it never speaks of entries a lane did not read.
// A redo reads the state again from memory, where it is still the launch's input.
#include "hm_welford_dev.h"
#include "hm_producer_rules.h"
#include <mutex>

namespace hm {

struct WelfordU16K {
    const uint16_t* frame[HM_MAX_FRAMES];
    const double* icrf;          // (2^b, C) or null
    double* mean;
    double* m2;                  // nullable
    int64_t n;
    int32_t n_frames, C;
    uint32_t mask, n_dn;         // M = 2^b - 1, 2^b
    double count0;               // frames already folded into mean / m2
    double max_dn, rcp_max;      // M and RN(1 / M)
    double rcp[HM_MAX_FRAMES];   // RN(1 / (count0 + k + 1)), formed on the host
};

constexpr int kWelfordU16LdsBlock = 1024;    // threads of the tab=lds workgroup: one per CU
constexpr int kWelfordU16Block = 256;
constexpr int kWelfordU16LdsHead = 16;       // bytes in front of the LDS table (the odd-table word)

// where f comes from: off = offset(channel) once per element, then at(DN & M, off) per frame
template <int PLACE> struct WelfordU16Src;
template <> struct WelfordU16Src<hm_rules::WELFORD_U16_LDS> {
    const double* t; uint32_t col;                          // col: 2^b with an ICRF, 0 for the one column dn / M
    __device__ __forceinline__ uint32_t offset(uint32_t c) const { return c * col; }
    __device__ __forceinline__ double at(uint32_t dn, uint32_t off) const { return t[dn + off]; }
};
template <> struct WelfordU16Src<hm_rules::WELFORD_U16_COMPUTED> {
    double max_dn, r;
    __device__ __forceinline__ uint32_t offset(uint32_t) const { return 0u; }
    __device__ __forceinline__ double at(uint32_t dn, uint32_t) const {
        const double d = static_cast<double>(dn), q0 = d * r;
        return fma(fma(-q0, max_dn, d), r, q0);             // == d / max_dn (file header)
    }
};
template <> struct WelfordU16Src<hm_rules::WELFORD_U16_GLOBAL> {
    const double* icrf; uint32_t C;
    __device__ __forceinline__ uint32_t offset(uint32_t c) const { return c; }
    __device__ __forceinline__ double at(uint32_t dn, uint32_t off) const { return icrf[dn * C + off]; }
};

// The gathers and the exact redo keep their own text beside hm_welford.hip's: every shared form tried moved a kernel.
// reference arithmetic with the IEEE division for `count` consecutive elements, all frames (rare path and odd tail)
template <bool M2, typename Src>
__device__ __forceinline__ void welford_u16_exact(const WelfordU16K& a, const Src& src, int64_t e0, int count, double* mean, double* m2) {
    for (int j = 0; j < count; ++j) {
        const int64_t e = e0 + j;
        const uint32_t off = src.offset(static_cast<uint32_t>(e % a.C));
        double m = a.mean[e], q = M2 ? a.m2[e] : 0.0, cnt = a.count0;
        for (int k = 0; k < a.n_frames; ++k) {
            cnt += 1.0;
            const double f = src.at(a.frame[k][e] & a.mask, off);
            const double delta = f - m;                                   // :205
            m = m + delta / cnt;                                          // :206
            if (M2) q = q + delta * (f - m);                              // :208
        }
        mean[j] = m; m2[j] = q;
    }
}

// G frames starting at k0 for the lane's two elements (fast division: the caller checks its range, hm_welford_dev.h).
template <bool M2, int G, bool VEC, int PLACE>
__device__ __forceinline__ bool welford_u16_group(const WelfordU16K& a, const WelfordU16Src<PLACE>& src, int k0, int64_t e, uint32_t off0,
                                                  uint32_t off1, double& cnt, double (&m)[2], double (&q)[2]) {
    uint32_t raw[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        const uint16_t* p = a.frame[k0 + k] + e;
        raw[k] = VEC ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p)) : (p[0] | (static_cast<uint32_t>(p[1]) << 16));
    }
    double f[G][2];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        f[k][0] = src.at(raw[k] & a.mask, off0);
        f[k][1] = src.at((raw[k] >> 16) & a.mask, off1);
    }
#define HM_WELFORD_TEST_GATHERED (PLACE == hm_rules::WELFORD_U16_GLOBAL)
#include "hm_welford_fold_body.h"
}

template <bool M2, int PLACE>
__global__ __launch_bounds__(PLACE == hm_rules::WELFORD_U16_LDS ? kWelfordU16LdsBlock : kWelfordU16Block) void k_welford_u16(const WelfordU16K a) {
    using namespace hm_rules;
    const uint32_t C = static_cast<uint32_t>(a.C);
    WelfordU16Src<PLACE> src;
    bool table_ok = true;
    if constexpr (PLACE == WELFORD_U16_LDS) {
        extern __shared__ __attribute__((aligned(16))) char lds[];
        uint32_t* odd_word = reinterpret_cast<uint32_t*>(lds);
        double* t = reinterpret_cast<double*>(lds + kWelfordU16LdsHead);
        const uint32_t cols = a.icrf ? C : 1u;
        if (threadIdx.x == 0) *odd_word = 0u;
        __syncthreads();
        bool odd = false;
        for (uint32_t i = threadIdx.x; i < a.n_dn * cols; i += blockDim.x) {    // t[c][dn]: the gather index is dn + 2^b c
            const uint32_t dn = i / cols, c = i - dn * cols;
            const double v = a.icrf ? a.icrf[i] : static_cast<double>(dn) / a.max_dn;
            t[c * a.n_dn + dn] = v;
            odd = odd || welford_entry_odd(v);
        }
        if (odd) atomicOr(odd_word, 1u);
        __syncthreads();
        table_ok = *odd_word == 0u;
        src.t = t; src.col = a.icrf ? a.n_dn : 0u;
    } else if constexpr (PLACE == WELFORD_U16_COMPUTED) {
        src.max_dn = a.max_dn; src.r = a.rcp_max;
    } else {
        src.icrf = a.icrf; src.C = C;
    }

#define HM_WELFORD_PAIR_ALIGN 4
#define HM_WELFORD_OFFSET(c) src.offset(c)
#define HM_WELFORD_GROUP(G, VEC) welford_u16_group<M2, G, VEC, PLACE>(a, src, k0, e, off0, off1, cnt, m, q)
#define HM_WELFORD_EXACT(e0, count) welford_u16_exact<M2>(a, src, e0, count, m, q)
#include "hm_welford_lane_body.h"
}

__global__ __launch_bounds__(256) void k_welford_finalize_u16(const double* __restrict__ mean, const double* __restrict__ m2, double count,
                                                              double max_dn, uint16_t* __restrict__ out_mean,
                                                              uint16_t* __restrict__ out_std, int64_t n) {
#define HM_WELFORD_SCALE max_dn
#include "hm_welford_finalize_body.h"
}

// More dynamic LDS than a kernel gets by default: both tab=lds instantiations are given the fit rule's table size and the head, once per
// process, on the first launch of either (host-side, no stream work).
static int welford_u16_lds_limit() {
    static std::once_flag once;
    static int status = HM_OK;
    std::call_once(once, [] {
        const void* fns[] = {reinterpret_cast<const void*>(&k_welford_u16<false, hm_rules::WELFORD_U16_LDS>),
                             reinterpret_cast<const void*>(&k_welford_u16<true, hm_rules::WELFORD_U16_LDS>)};
        for (const void* fn : fns)
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(hm_rules::kWelfordU16LdsTableBytes) + kWelfordU16LdsHead) != hipSuccess) {
                (void)hipGetLastError();
                status = HM_ELAUNCH;
            }
    });
    return status;
}

static const char* welford_u16_tab_name(int place) {
    return place == hm_rules::WELFORD_U16_LDS ? "lds" : place == hm_rules::WELFORD_U16_COMPUTED ? "computed" : "global";
}

}  // namespace hm

using namespace hm;

extern "C" int hm_welford_update_u16(const void* const* frames, int n_frames, int64_t count_before, const double* icrf, double* mean,
                                     double* m2, int64_t n_elems, int C, int bit_depth, int variant, void* stream) {
    using namespace hm_rules;
    bool empty;
    const int rc = check_welford_update_u16(frames, n_frames, count_before, icrf, mean, n_elems, C, bit_depth, variant, empty);
    if (rc != HM_OK || empty) return rc;
    const int place = variant != WELFORD_U16_AUTO ? variant : welford_u16_default_placement(bit_depth, C, icrf != nullptr);
    WelfordU16K k{};
    for (int i = 0; i < n_frames; ++i) k.frame[i] = static_cast<const uint16_t*>(frames[i]);
    k.icrf = icrf; k.mean = mean; k.m2 = m2; k.n = n_elems; k.n_frames = n_frames; k.C = C;
    k.n_dn = 1u << bit_depth; k.mask = k.n_dn - 1u;
    k.count0 = static_cast<double>(count_before);
    k.max_dn = static_cast<double>(k.mask); k.rcp_max = 1.0 / k.max_dn;
    for (int i = 0; i < n_frames; ++i) k.rcp[i] = 1.0 / (k.count0 + static_cast<double>(i + 1));
    const int64_t units = (n_elems + 1) / 2;
    hipStream_t st = as_stream(stream);
#define HM_WELFORD_U16_LAUNCH(P, grid, block, lds) \
    do { if (m2) hipLaunchKernelGGL((k_welford_u16<true, P>), dim3(grid), dim3(block), lds, st, k); \
         else hipLaunchKernelGGL((k_welford_u16<false, P>), dim3(grid), dim3(block), lds, st, k); } while (0)
    if (place == WELFORD_U16_LDS) {
        const int lrc = welford_u16_lds_limit();
        if (lrc != HM_OK) return lrc;
        const unsigned lds = static_cast<unsigned>(welford_u16_table_bytes(bit_depth, C, icrf != nullptr)) + kWelfordU16LdsHead;
        const unsigned grid = stream_grid(units, kWelfordU16LdsBlock, 1);         // one workgroup per CU at the most
        HM_WELFORD_U16_LAUNCH(WELFORD_U16_LDS, grid, kWelfordU16LdsBlock, lds);
    } else {
        const unsigned grid = stream_grid(units, kWelfordU16Block, 8);
        if (place == WELFORD_U16_COMPUTED) HM_WELFORD_U16_LAUNCH(WELFORD_U16_COMPUTED, grid, kWelfordU16Block, 0);
        else HM_WELFORD_U16_LAUNCH(WELFORD_U16_GLOBAL, grid, kWelfordU16Block, 0);
    }
#undef HM_WELFORD_U16_LAUNCH
    return launch_status();
}

extern "C" int hm_welford_update_u16_describe(int64_t n_elems, int n_frames, int C, int with_icrf, int with_m2, int bit_depth, int variant,
                                              char* buf, int buf_len) {
    using namespace hm_rules;
    if (!buf || buf_len < 1) return HM_EINVAL;
    buf[0] = '\0';
    bool empty;
    const int rc = check_welford_update_u16_counts(n_frames, 0, n_elems, C, with_icrf != 0, bit_depth, variant, empty);
    if (rc != HM_OK || empty) return rc;
    const int place = variant != WELFORD_U16_AUTO ? variant : welford_u16_default_placement(bit_depth, C, with_icrf != 0);
    snprintf(buf, static_cast<size_t>(buf_len), "k_welford_u16<m2=%d,tab=%s,bits=%d>", with_m2 != 0, welford_u16_tab_name(place), bit_depth);
    return HM_OK;
}

extern "C" int hm_welford_finalize_u16(const double* mean, const double* m2, int64_t count, int bit_depth, uint16_t* out_mean,
                                       uint16_t* out_std, int64_t n_elems, void* stream) {
    bool empty;
    const int rc = hm_rules::check_welford_finalize_u16(mean, m2, count, bit_depth, out_mean, out_std, n_elems, empty);
    if (rc != HM_OK || empty) return rc;
    const unsigned grid = stream_grid(n_elems, 256, 8);
    hipLaunchKernelGGL(k_welford_finalize_u16, dim3(grid), dim3(256), 0, as_stream(stream), mean, m2, static_cast<double>(count),
                       static_cast<double>((1 << bit_depth) - 1), out_mean, out_std, n_elems);
    return launch_status();
}

extern "C" int64_t hm_welford_u16_algorithmic_bytes(int n_frames, int with_m2, int64_t n_elems) {
    return hm_rules::welford_algorithmic_bytes(2, n_frames, with_m2 != 0, n_elems);
}
