// hm_noise_u16.hip - the per-DN STD table of 9- to 16-bit cameras from per-level noise moments (gfx950): uint16 HWC frames with an explicit
// bit depth b, M = 2^b - 1 (hdrmerge.h: hm_noise_moments_update_u16, hm_noise_moments_std). hm_noise.hip's joint histogram is (2^b, 2^b, C)
// at depth b - 96 GiB at 16 bits - but _calculate_STD (modules/video_processing.py:109-133) reduces each of its rows to a count, a mean and a
// centred second moment, and three integers per (mean level, channel) carry exactly that:
//
//   for every frame and element e, m = mean[e] & M, f = frame[e] & M, c = e % C, d = f - m:
//       moments[m][c][0] += 1;   moments[m][c][1] += d;   moments[m][c][2] += d * d            (int64, modulo 2^64)
//   hm_noise_moments_std:  std[m][c] = sqrt(n S2 - S1^2) / n / M, the numerator exact in 128-bit integers (hm_producer_math.h)
//
// The sums are integers, so the result does not depend on the order of the atomics: it is exact, like the 8-bit profile's counts.
//
// k_noise_moments_u16<C, PLACE> keeps k_noise_profile's geometry: one lane owns one 16-byte unit - eight uint16 elements - for all frames
// of the launch (non-temporal 16-byte loads, four frames in flight; 2-byte loads when a pointer is not 16-byte aligned and in the ragged
// tail). Its mean DNs are loaded once, and across the frames it keeps sum d (int32: 32 * 65535 < 2^21) and sum d^2 (64 bits: d^2 < 2^32,
// 32 of them < 2^37) of each element in registers. After the last frame it adds ONE triple per element - not one per element-frame, 32
// times fewer adds than a histogram needs - and elements of the lane that share level and channel (positions j, j + C, ...) are merged in
// registers first, as noise_unit merges its runs: a flat region costs a lane C adds, not eight.
//
// PLACE (hm_rules::NoiseMomentsTab; the fit rule and the default are hm_producer_rules.h's) says where the triples go:
//   tab=lds     every workgroup (1024 threads, one per CU) privatises the whole (2^b, C) table in dynamic LDS as three arrays - u64 sum d^2,
//               i64 sum d, u32 ELEMENT count, 20 bytes per level and channel - with ds_add_u64 / ds_add_u32, and flushes its non-zero
//               entries once per launch with 8-byte global atomics; the frame count is multiplied into the count there. The 64-bit LDS
//               sums may wrap: they are added modulo 2^64, which is the output's own arithmetic. The u32 count must not: the host raises
//               the grid so that a workgroup sees fewer than 2^32 elements, as hm_noise_profile_update does.
//   tab=global  the triples go straight to 8-byte global atomics on `moments` (global_atomic_add_x2, no compare-and-swap loop);
//               256-thread workgroups.
//   tab=window  for the depths whose table does not fit: a window of kNoiseMomentsWindowSlots slots in LDS over the levels a workgroup
//               actually meets (1024 threads, one workgroup per CU). Slot = hash(level * C + c); a triple claims an empty slot for its key
//               with one LDS compare-and-swap, adds to a slot that already has its key, and goes to the global atomics when another key
//               holds the slot. The window is flushed - 8-byte global atomics for the claimed slots - and cleared after EVERY pass of the
//               workgroup's grid-stride loop (8192 consecutive elements), so that it follows the image: the levels of one pass are
//               neighbours in the scene. Every triple is added exactly once, in the window or in memory.
#include "hm_common.h"
#include "hm_producer_math.h"
#include "hm_producer_rules.h"
#include <mutex>

namespace hm {

constexpr int kMomentsLdsBlock = 1024;         // threads of the tab=lds workgroup: one per CU
constexpr int kMomentsBlock = 256;
constexpr int kMomentsUnit = 8;                // elements per lane and unit (one uint4 per frame)
constexpr int kMomentsGroup = 4;               // frames loaded before they are folded: 64 bytes in flight per lane

typedef uint32_t mom_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long mom_u64;

struct NoiseMomentsK {
    const uint16_t* frame[HM_MAX_FRAMES];
    const uint16_t* mean;
    mom_u64* mom;                              // (2^b, C, 3) int64
    int64_t n;
    int32_t n_frames;
    uint32_t mask, n_dn;                       // M = 2^b - 1, 2^b
};

// where a triple goes: `elems` elements of level m and channel c with their sums over the launch's frames
template <int C, int PLACE> struct NoiseMomentsSink;
template <int C> struct NoiseMomentsSink<C, hm_rules::NOISE_MOMENTS_LDS> {
    mom_u64* s2; mom_u64* s1; uint32_t* cnt;   // LDS, (2^b * C) entries each
    __device__ __forceinline__ void add(uint32_t m, uint32_t c, uint32_t elems, int32_t d1, mom_u64 d2) const {
        const uint32_t i = m * C + c;
        atomicAdd(&cnt[i], elems);
        if (d2 != 0) {                                             // d2 == 0 means every d was 0: a flat region adds its count only
            atomicAdd(&s2[i], d2);
            if (d1 != 0) atomicAdd(&s1[i], static_cast<mom_u64>(static_cast<long long>(d1)));
        }
    }
};
template <int C> struct NoiseMomentsSink<C, hm_rules::NOISE_MOMENTS_GLOBAL> {
    mom_u64* mom; uint32_t n_frames;
    __device__ __forceinline__ void add(uint32_t m, uint32_t c, uint32_t elems, int32_t d1, mom_u64 d2) const {
        mom_u64* p = mom + static_cast<int64_t>(m * C + c) * 3;
        atomicAdd(p, static_cast<mom_u64>(elems) * n_frames);
        if (d2 != 0) {
            atomicAdd(p + 2, d2);
            if (d1 != 0) atomicAdd(p + 1, static_cast<mom_u64>(static_cast<long long>(d1)));
        }
    }
};

constexpr uint32_t kMomentsWindowEmpty = 0xffffffffu;                  // no key: keys are level * C + c < 2^18
template <int C> struct NoiseMomentsSink<C, hm_rules::NOISE_MOMENTS_WINDOW> {
    mom_u64* s2; mom_u64* s1; uint32_t* cnt; uint32_t* key;           // LDS, kNoiseMomentsWindowSlots entries each
    NoiseMomentsSink<C, hm_rules::NOISE_MOMENTS_GLOBAL> memory;
    __device__ __forceinline__ void add(uint32_t m, uint32_t c, uint32_t elems, int32_t d1, mom_u64 d2) const {
        const uint32_t i = m * C + c;
        const uint32_t slot = (i * 2654435761u) >> (32 - hm_rules::kNoiseMomentsWindowBits);
        const uint32_t prev = atomicCAS(&key[slot], kMomentsWindowEmpty, i);
        if (prev == kMomentsWindowEmpty || prev == i) {
            atomicAdd(&cnt[slot], elems);
            if (d2 != 0) {
                atomicAdd(&s2[slot], d2);
                if (d1 != 0) atomicAdd(&s1[slot], static_cast<mom_u64>(static_cast<long long>(d1)));
            }
        } else {
            memory.add(m, c, elems, d1, d2);
        }
    }
};

// the eight DNs of one 16-byte word, masked
__device__ __forceinline__ void moments_unpack(const mom_u32x4 w, uint32_t mask, uint32_t (&dn)[kMomentsUnit]) {
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < kMomentsUnit; ++j) dn[j] = ((j & 1) ? ws[j >> 1] >> 16 : ws[j >> 1]) & mask;
}

__device__ __forceinline__ void moments_fold(const uint32_t (&fv)[kMomentsUnit], const uint32_t (&mv)[kMomentsUnit], int32_t (&s1)[kMomentsUnit],
                                             mom_u64 (&s2)[kMomentsUnit]) {
#pragma unroll
    for (int j = 0; j < kMomentsUnit; ++j) {
        const uint32_t d = fv[j] - mv[j];                          // two's complement; |d| <= 65535: d^2 < 2^32, the low word of d * d
        s1[j] += static_cast<int32_t>(d);
        s2[j] += d * d;
    }
}

// one unit of `valid` (<= 8) consecutive elements starting at e0, every frame; VEC: 16-byte loads (all 8 valid, every pointer aligned)
template <int C, bool VEC, typename Sink>
__device__ __forceinline__ void moments_unit(const NoiseMomentsK& a, const Sink& sink, int64_t e0, int valid) {
    uint32_t mv[kMomentsUnit];
    int32_t s1[kMomentsUnit];
    mom_u64 s2[kMomentsUnit];
#pragma unroll
    for (int j = 0; j < kMomentsUnit; ++j) { s1[j] = 0; s2[j] = 0; }
    if (VEC) {
        moments_unpack(*reinterpret_cast<const mom_u32x4*>(a.mean + e0), a.mask, mv);
        int k = 0;
        for (; k + kMomentsGroup <= a.n_frames; k += kMomentsGroup) {
            mom_u32x4 w[kMomentsGroup];
#pragma unroll
            for (int q = 0; q < kMomentsGroup; ++q) w[q] = __builtin_nontemporal_load(reinterpret_cast<const mom_u32x4*>(a.frame[k + q] + e0));
#pragma unroll
            for (int q = 0; q < kMomentsGroup; ++q) {
                uint32_t fv[kMomentsUnit];
                moments_unpack(w[q], a.mask, fv);
                moments_fold(fv, mv, s1, s2);
            }
        }
        for (; k < a.n_frames; ++k) {
            uint32_t fv[kMomentsUnit];
            moments_unpack(__builtin_nontemporal_load(reinterpret_cast<const mom_u32x4*>(a.frame[k] + e0)), a.mask, fv);
            moments_fold(fv, mv, s1, s2);
        }
    } else {
#pragma unroll
        for (int j = 0; j < kMomentsUnit; ++j) mv[j] = j < valid ? a.mean[e0 + j] & a.mask : 0u;
        for (int k = 0; k < a.n_frames; ++k) {
            uint32_t fv[kMomentsUnit];
#pragma unroll
            for (int j = 0; j < kMomentsUnit; ++j) fv[j] = j < valid ? a.frame[k][e0 + j] & a.mask : 0u;
            moments_fold(fv, mv, s1, s2);
        }
    }
    // one triple per (level, channel) of the lane: position j takes every later position j + C, j + 2C, ... of its level with it
    const uint32_t c0 = static_cast<uint32_t>(e0 % C);
    bool taken[kMomentsUnit];
#pragma unroll
    for (int j = 0; j < kMomentsUnit; ++j) taken[j] = !(VEC || j < valid);
#pragma unroll
    for (int j = 0; j < kMomentsUnit; ++j) {
        if (taken[j]) continue;
        uint32_t elems = 1;
        int32_t d1 = s1[j];                                        // eight elements: 8 * 2^21 = 2^24
        mom_u64 d2 = s2[j];
#pragma unroll
        for (int i = j + C; i < kMomentsUnit; i += C) {
            if (!taken[i] && mv[i] == mv[j]) {
                taken[i] = true;
                elems += 1; d1 += s1[i]; d2 += s2[i];
            }
        }
        sink.add(mv[j], (c0 + static_cast<uint32_t>(j)) % C, elems, d1, d2);
    }
}

template <int C, int PLACE>
__global__ __launch_bounds__(PLACE == hm_rules::NOISE_MOMENTS_GLOBAL ? kMomentsBlock : kMomentsLdsBlock) void k_noise_moments_u16(const NoiseMomentsK a) {
    using namespace hm_rules;
    NoiseMomentsSink<C, PLACE> sink;
    const uint32_t n_ent = a.n_dn * C;
    if constexpr (PLACE == NOISE_MOMENTS_LDS) {
        extern __shared__ __attribute__((aligned(16))) char lds[];
        sink.s2 = reinterpret_cast<mom_u64*>(lds);
        sink.s1 = sink.s2 + n_ent;
        sink.cnt = reinterpret_cast<uint32_t*>(sink.s1 + n_ent);
        uint32_t* words = reinterpret_cast<uint32_t*>(lds);
        for (uint32_t i = threadIdx.x; i < n_ent * 5u; i += blockDim.x) words[i] = 0u;
        __syncthreads();
    } else if constexpr (PLACE == NOISE_MOMENTS_WINDOW) {
        extern __shared__ __attribute__((aligned(16))) char lds[];
        sink.s2 = reinterpret_cast<mom_u64*>(lds);
        sink.s1 = sink.s2 + kNoiseMomentsWindowSlots;
        sink.cnt = reinterpret_cast<uint32_t*>(sink.s1 + kNoiseMomentsWindowSlots);
        sink.key = sink.cnt + kNoiseMomentsWindowSlots;
        sink.memory.mom = a.mom; sink.memory.n_frames = static_cast<uint32_t>(a.n_frames);
        for (uint32_t i = threadIdx.x; i < kNoiseMomentsWindowSlots; i += blockDim.x) {
            sink.s2[i] = 0; sink.s1[i] = 0; sink.cnt[i] = 0u; sink.key[i] = kMomentsWindowEmpty;
        }
        __syncthreads();
    } else {
        sink.mom = a.mom; sink.n_frames = static_cast<uint32_t>(a.n_frames);
    }

    bool vec = aligned_dev(a.mean, 16);
    for (int k = 0; k < a.n_frames; ++k) vec = vec && aligned_dev(a.frame[k], 16);
    const int64_t units = (a.n + kMomentsUnit - 1) / kMomentsUnit;
    const int64_t full = a.n / kMomentsUnit;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    auto unit = [&](int64_t u) {
        const int64_t e0 = u * kMomentsUnit;
        if (vec && u < full) moments_unit<C, true>(a, sink, e0, kMomentsUnit);
        else moments_unit<C, false>(a, sink, e0, static_cast<int>(a.n - e0 < kMomentsUnit ? a.n - e0 : kMomentsUnit));
    };

    if constexpr (PLACE == NOISE_MOMENTS_WINDOW) {
        // `base` is the workgroup's: every lane makes every pass and meets both barriers
        for (int64_t base = static_cast<int64_t>(blockIdx.x) * blockDim.x; base < units; base += stride) {
            if (base + threadIdx.x < units) unit(base + threadIdx.x);
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < kNoiseMomentsWindowSlots; i += blockDim.x) {      // flush and clear the claimed slots
                const uint32_t key = sink.key[i];
                if (key == kMomentsWindowEmpty) continue;
                mom_u64* p = a.mom + static_cast<int64_t>(key) * 3;
                atomicAdd(p, static_cast<mom_u64>(sink.cnt[i]) * static_cast<uint32_t>(a.n_frames));
                const mom_u64 d2 = sink.s2[i];
                if (d2 != 0) {
                    atomicAdd(p + 2, d2);
                    const mom_u64 d1 = sink.s1[i];
                    if (d1 != 0) atomicAdd(p + 1, d1);
                }
                sink.s2[i] = 0; sink.s1[i] = 0; sink.cnt[i] = 0u; sink.key[i] = kMomentsWindowEmpty;
            }
            __syncthreads();
        }
    } else {
        for (int64_t u = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; u < units; u += stride) unit(u);
    }

    if constexpr (PLACE == NOISE_MOMENTS_LDS) {
        __syncthreads();
        // flush: entry i = level * C + c  ->  moments[i][0..2]; an entry without elements has no sums
        for (uint32_t i = threadIdx.x; i < n_ent; i += blockDim.x) {
            const uint32_t elems = sink.cnt[i];
            if (elems == 0u) continue;
            mom_u64* p = a.mom + static_cast<int64_t>(i) * 3;
            atomicAdd(p, static_cast<mom_u64>(elems) * static_cast<uint32_t>(a.n_frames));
            const mom_u64 d2 = sink.s2[i];
            if (d2 != 0) {
                atomicAdd(p + 2, d2);
                const mom_u64 d1 = sink.s1[i];
                if (d1 != 0) atomicAdd(p + 1, d1);
            }
        }
    }
}

// one lane per (level, channel): noise_moments_level_std of hm_producer_math.h
__global__ __launch_bounds__(256) void k_noise_moments_std(const long long* __restrict__ mom, int n_ent, double max_dn, double* __restrict__ out) {
    const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n_ent) return;
    const long long* t = mom + static_cast<int64_t>(i) * 3;
    out[i] = noise_moments_level_std(t[0], t[1], t[2], max_dn);
}

// More dynamic LDS than a kernel gets by default: the tab=lds and tab=window instantiations are given the fit rule's table size (the window,
// 96 KiB, is below it), once per process, on the first launch of one of them (host-side, no stream work).
static int noise_moments_lds_limit() {
    static std::once_flag once;
    static int status = HM_OK;
    std::call_once(once, [] {
        const void* fns[] = {reinterpret_cast<const void*>(&k_noise_moments_u16<1, hm_rules::NOISE_MOMENTS_LDS>),
                             reinterpret_cast<const void*>(&k_noise_moments_u16<2, hm_rules::NOISE_MOMENTS_LDS>),
                             reinterpret_cast<const void*>(&k_noise_moments_u16<3, hm_rules::NOISE_MOMENTS_LDS>),
                             reinterpret_cast<const void*>(&k_noise_moments_u16<4, hm_rules::NOISE_MOMENTS_LDS>),
                             reinterpret_cast<const void*>(&k_noise_moments_u16<1, hm_rules::NOISE_MOMENTS_WINDOW>),
                             reinterpret_cast<const void*>(&k_noise_moments_u16<2, hm_rules::NOISE_MOMENTS_WINDOW>),
                             reinterpret_cast<const void*>(&k_noise_moments_u16<3, hm_rules::NOISE_MOMENTS_WINDOW>),
                             reinterpret_cast<const void*>(&k_noise_moments_u16<4, hm_rules::NOISE_MOMENTS_WINDOW>)};
        for (const void* fn : fns)
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(hm_rules::kNoiseMomentsLdsTableBytes)) !=
                hipSuccess) {
                (void)hipGetLastError();
                status = HM_ELAUNCH;
            }
    });
    return status;
}

template <int PLACE>
static void noise_moments_launch(int C, unsigned grid, unsigned block, unsigned lds, hipStream_t st, const NoiseMomentsK& k) {
    switch (C) {
        case 1: hipLaunchKernelGGL((k_noise_moments_u16<1, PLACE>), dim3(grid), dim3(block), lds, st, k); break;
        case 2: hipLaunchKernelGGL((k_noise_moments_u16<2, PLACE>), dim3(grid), dim3(block), lds, st, k); break;
        case 3: hipLaunchKernelGGL((k_noise_moments_u16<3, PLACE>), dim3(grid), dim3(block), lds, st, k); break;
        default: hipLaunchKernelGGL((k_noise_moments_u16<4, PLACE>), dim3(grid), dim3(block), lds, st, k); break;
    }
}

}  // namespace hm

using namespace hm;

extern "C" int64_t hm_noise_moments_algorithmic_bytes(int n_frames, int64_t n_elems, int C, int bit_depth) {
    return hm_rules::noise_moments_algorithmic_bytes(n_frames, n_elems, C, bit_depth);
}

extern "C" int hm_noise_moments_update_u16(const void* const* frames, int n_frames, const uint16_t* mean, int64_t n_elems, int C, int bit_depth,
                                           int64_t* moments, int variant, void* stream) {
    using namespace hm_rules;
    bool empty;
    const int rc = check_noise_moments_update(frames, n_frames, mean, n_elems, C, bit_depth, moments, variant, empty);
    if (rc != HM_OK || empty) return rc;
    const int place = variant != NOISE_MOMENTS_AUTO ? variant : noise_moments_default_placement(bit_depth, C);
    NoiseMomentsK k{};
    for (int i = 0; i < n_frames; ++i) k.frame[i] = static_cast<const uint16_t*>(frames[i]);
    k.mean = mean; k.mom = reinterpret_cast<mom_u64*>(moments); k.n = n_elems; k.n_frames = n_frames;
    k.n_dn = 1u << bit_depth; k.mask = k.n_dn - 1u;
    const int64_t units = (n_elems + kMomentsUnit - 1) / kMomentsUnit;
    hipStream_t st = as_stream(stream);
    if (place == NOISE_MOMENTS_LDS) {
        const int lrc = noise_moments_lds_limit();
        if (lrc != HM_OK) return lrc;
        // one workgroup per CU; more where a workgroup's element counters could reach 2^32 (units per lane x 8 x 1024 lanes)
        const int64_t max_units_per_lane = ((int64_t{1} << 32) - 1) / (int64_t{kMomentsUnit} * kMomentsLdsBlock);
        int64_t grid = stream_grid(units, kMomentsLdsBlock, 1);
        if ((units + grid * kMomentsLdsBlock - 1) / (grid * kMomentsLdsBlock) > max_units_per_lane)
            grid = (units + max_units_per_lane * kMomentsLdsBlock - 1) / (max_units_per_lane * kMomentsLdsBlock);
        if (grid > 0x7fffffff) return HM_EUNSUPPORTED;                        // this build's own: the launch grid's limit
        noise_moments_launch<NOISE_MOMENTS_LDS>(C, static_cast<unsigned>(grid), kMomentsLdsBlock,
                                                static_cast<unsigned>(noise_moments_table_bytes(bit_depth, C)), st, k);
    } else if (place == NOISE_MOMENTS_WINDOW) {
        const int lrc = noise_moments_lds_limit();
        if (lrc != HM_OK) return lrc;
        static_assert(kNoiseMomentsWindowBytes <= kNoiseMomentsLdsTableBytes, "the window takes the LDS table's budget");
        noise_moments_launch<NOISE_MOMENTS_WINDOW>(C, stream_grid(units, kMomentsLdsBlock, 1), kMomentsLdsBlock,
                                                   static_cast<unsigned>(kNoiseMomentsWindowBytes), st, k);
    } else {
        noise_moments_launch<NOISE_MOMENTS_GLOBAL>(C, stream_grid(units, kMomentsBlock, 8), kMomentsBlock, 0, st, k);
    }
    return launch_status();
}

extern "C" int hm_noise_moments_update_u16_describe(int64_t n_elems, int n_frames, int C, int bit_depth, int variant, char* buf, int buf_len) {
    using namespace hm_rules;
    if (!buf || buf_len < 1) return HM_EINVAL;
    buf[0] = '\0';
    const int rc = check_noise_moments_update_counts(n_frames, n_elems, C, bit_depth, variant);
    if (rc != HM_OK || n_frames == 0 || n_elems == 0) return rc;
    const int place = variant != NOISE_MOMENTS_AUTO ? variant : noise_moments_default_placement(bit_depth, C);
    snprintf(buf, static_cast<size_t>(buf_len), "k_noise_moments_u16<C=%d,tab=%s,bits=%d>", C,
             place == NOISE_MOMENTS_LDS ? "lds" : place == NOISE_MOMENTS_WINDOW ? "window" : "global",
             bit_depth);
    return HM_OK;
}

extern "C" int hm_noise_moments_std(const int64_t* moments, int C, int bit_depth, double* out_std, void* stream) {
    const int rc = hm_rules::check_noise_moments_std(moments, C, bit_depth, out_std);
    if (rc != HM_OK) return rc;
    const int n_ent = (1 << bit_depth) * C;
    hipLaunchKernelGGL(k_noise_moments_std, dim3((n_ent + 255) / 256), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const long long*>(moments), n_ent, static_cast<double>((1 << bit_depth) - 1), out_std);
    return launch_status();
}
