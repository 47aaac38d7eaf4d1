// hm_noise.hip - camera noise profiles and the per-DN STD table (gfx950): compute_noise_profiles, _calculate_STD and
// clean_data_edges of modules/video_processing.py:12-133.
//
//   profile[m, f, c] += 1 for every frame and element, m = mean frame DN, f = frame DN, c = e % C   (:77-106, np.add.at)
//
// k_noise_profile is a joint 2-D histogram over a stream of frames. The full 256 x 256 u32 histogram is 256 KiB per channel,
// more than a CU's 160 KiB of LDS, but noise keeps f near m: every workgroup privatises the BAND diagonals
// d = f - m + kNoiseHalfBand in [0, kNoiseBand) in LDS (u32, C x 32 KiB) and sends the rare element outside the band
// straight to a 64-bit global atomic on the output. Counts are integers, so the result does not depend on the order of the
// atomics: it is exact.
//   - one lane owns 16 consecutive elements (one 16-byte load per frame) for all frames of the launch. Its mean DNs are fixed,
//     so a run of equal frame DNs of one element is counted in a register and added once (a saturated or flat region would
//     otherwise put 32 frames x many lanes on one LDS word);
//   - one 1024-thread workgroup per CU (the band takes 96 KiB at C = 3), grid-stride over the 16-element units;
//   - the flush adds the non-zero band counters to the output once per workgroup and launch (8-byte atomics on rows of
//     the output that are contiguous per mean level: LDS layout [m][d][c] = global layout [m][m - half + d][c]).
// Bound: a workgroup counts at most units_per_lane x 16 x n_frames x 1024 < 2^32 elements per launch (checked on the host).
#include "hm_common.h"
#include "hm_producer_math.h"
#include "hm_producer_rules.h"

namespace hm {

constexpr int kNoiseBand = 32;                 // diagonals kept in LDS per (m, c)
constexpr int kNoiseHalfBand = 16;             // d = f - m + 16: f in [m - 16, m + 15]
constexpr int kNoiseBlock = 1024;
constexpr int kNoiseUnit = 16;                 // elements per lane and unit (one uint4 per frame)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct NoiseK {
    const uint8_t* frame[HM_MAX_FRAMES];
    const uint8_t* mean;
    unsigned long long* prof;                  // (256, 256, C) int64
    int64_t n;
    int32_t n_frames;
};

template <int C>
__device__ __forceinline__ void noise_count(uint32_t* h, unsigned long long* prof, uint32_t m, uint32_t c, uint32_t f, uint32_t cnt) {
    const uint32_t d = f - m + kNoiseHalfBand;
    if (d < static_cast<uint32_t>(kNoiseBand)) {
        atomicAdd(&h[(m * kNoiseBand + d) * C + c], cnt);
    } else {
        atomicAdd(&prof[(m * 256u + f) * C + c], static_cast<unsigned long long>(cnt));     // outside the band: rare
    }
}

// one unit of `valid` (<= 16) consecutive elements starting at e0, every frame; VEC: 16-byte loads (all 16 valid, aligned)
template <int C, bool VEC>
__device__ __forceinline__ void noise_unit(const NoiseK& a, uint32_t* h, int64_t e0, int valid) {
    uint32_t mv[kNoiseUnit], st[kNoiseUnit];                       // st = current frame DN | run length << 8
    uint32_t c0 = static_cast<uint32_t>(e0 % C);
    if (VEC) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(a.mean + e0);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < kNoiseUnit; ++j) mv[j] = (ws[j >> 2] >> (8 * (j & 3))) & 255u;
    } else {
#pragma unroll
        for (int j = 0; j < kNoiseUnit; ++j) mv[j] = j < valid ? a.mean[e0 + j] : 0u;
    }
    auto frame_dn = [&](int k, uint32_t (&fv)[kNoiseUnit]) {
        if (VEC) {
            const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.frame[k] + e0));
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < kNoiseUnit; ++j) fv[j] = (ws[j >> 2] >> (8 * (j & 3))) & 255u;
        } else {
#pragma unroll
            for (int j = 0; j < kNoiseUnit; ++j) fv[j] = j < valid ? a.frame[k][e0 + j] : 0u;
        }
    };
    {
        uint32_t fv[kNoiseUnit];
        frame_dn(0, fv);
#pragma unroll
        for (int j = 0; j < kNoiseUnit; ++j) st[j] = fv[j] | 256u;
    }
    for (int k = 1; k < a.n_frames; ++k) {
        uint32_t fv[kNoiseUnit];
        frame_dn(k, fv);
        uint32_t c = c0;
#pragma unroll
        for (int j = 0; j < kNoiseUnit; ++j) {
            if ((st[j] & 255u) == fv[j]) {
                st[j] += 256u;
            } else {
                if (VEC || j < valid) noise_count<C>(h, a.prof, mv[j], c, st[j] & 255u, st[j] >> 8);
                st[j] = fv[j] | 256u;
            }
            c = (c + 1u == C) ? 0u : c + 1u;
        }
    }
    uint32_t c = c0;
#pragma unroll
    for (int j = 0; j < kNoiseUnit; ++j) {
        if (VEC || j < valid) noise_count<C>(h, a.prof, mv[j], c, st[j] & 255u, st[j] >> 8);
        c = (c + 1u == C) ? 0u : c + 1u;
    }
}

template <int C>
__global__ __launch_bounds__(kNoiseBlock) void k_noise_profile(const NoiseK a) {
    __shared__ uint32_t h[256 * kNoiseBand * C];
    for (int i = threadIdx.x; i < 256 * kNoiseBand * C; i += kNoiseBlock) h[i] = 0u;
    __syncthreads();

    bool vec = aligned_dev(a.mean, 16);
    for (int k = 0; k < a.n_frames; ++k) vec = vec && aligned_dev(a.frame[k], 16);
    const int64_t units = (a.n + kNoiseUnit - 1) / kNoiseUnit;
    const int64_t full = a.n / kNoiseUnit;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kNoiseBlock;
    for (int64_t u = static_cast<int64_t>(blockIdx.x) * kNoiseBlock + threadIdx.x; u < units; u += stride) {
        const int64_t e0 = u * kNoiseUnit;
        if (vec && u < full) noise_unit<C, true>(a, h, e0, kNoiseUnit);
        else noise_unit<C, false>(a, h, e0, static_cast<int>(a.n - e0 < kNoiseUnit ? a.n - e0 : kNoiseUnit));
    }
    __syncthreads();

    // flush: counter i = (m * BAND + d) * C + c  ->  output ((m * 256 + m - half + d) * C + c); zeros are skipped
    for (int i = threadIdx.x; i < 256 * kNoiseBand * C; i += kNoiseBlock) {
        const uint32_t v = h[i];
        if (v == 0u) continue;
        const int m = i / (kNoiseBand * C);
        const int r = i - m * (kNoiseBand * C);                    // d * C + c
        const int f = m - kNoiseHalfBand + r / C;                  // in [0, 255] whenever v != 0
        atomicAdd(&a.prof[static_cast<int64_t>(m * 256 + f) * C + r % C], static_cast<unsigned long long>(v));
    }
}

// _calculate_STD (:109-133) for one (level i, channel c) per wave: edges = linspace(0, 1, 256) from the caller; over the non-zero
// bins, mean = sum(h * edges) / sum(h) and std = sqrt(sum((edges - mean)^2 h) / sum(h)); an empty row gives 0 / 0 = NaN.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_noise_std(const long long* __restrict__ prof, int C, const double* __restrict__ edges,
                                                   double* __restrict__ out) {
    const int wave = static_cast<int>((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (wave >= 256 * C) return;
    const int i = wave / C, c = wave % C;
    double hv[4], ev[4], cnt = 0.0, s1 = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int b = q * 64 + lane;
        hv[q] = static_cast<double>(prof[(static_cast<int64_t>(i) * 256 + b) * C + c]);
        ev[q] = edges[b];
        cnt += hv[q];
        if (hv[q] != 0.0) s1 += hv[q] * ev[q];
    }
    cnt = wave_sum_f64(cnt);
    const double mean = wave_sum_f64(s1) / cnt;
    double s2 = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (hv[q] != 0.0) {
            const double dv = ev[q] - mean;
            s2 += (dv * dv) * hv[q];
        }
    }
    s2 = wave_sum_f64(s2);
    if (lane == 0) out[i * C + c] = sqrt(s2 / cnt);
}

// clean_data_edges (:12-74): one lane per (row i, channel c), the reference's four integer passes in order, in place. The passes are
// clean_edges_row() of hm_producer_math.h written out: called here, the kernel's code changes.
__global__ __launch_bounds__(64) void k_noise_clean_edges(long long* __restrict__ prof, int C) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 256 * C) return;
    const int i = t / C, c = t % C;
    long long* row = prof + static_cast<int64_t>(i) * 256 * C + c;
    auto D = [&](int m) -> long long& { return row[static_cast<int64_t>(m) * C]; };
    const int center = i, min_dn = 0, max_dn = 255;
    for (int m = center - 1; m > min_dn; --m) {                                    // :31-38
        if (D(m) == 0 && D(m - 1) == 0) { for (int q = 0; q < m; ++q) D(q) = 0; break; }
        if (D(m - 1) >= D(m) || D(m + 1) <= D(m)) D(m) = floordiv2(D(m - 1) + D(m + 1));
    }
    for (int m = center + 1; m < max_dn; ++m) {                                    // :41-48
        if (D(m) == 0 && D(m + 1) == 0) { for (int q = m; q < 256; ++q) D(q) = 0; break; }
        if (D(m + 1) >= D(m) || D(m - 1) <= D(m)) D(m) = floordiv2(D(m - 1) + D(m + 1));
    }
    for (int m = min_dn + 1; m < center;) {                                        // :51-58
        if (D(m) == 0 && D(m - 1) != 0 && D(m + 1) != 0) D(m) = D(m - 1);
        else if (D(m) == D(m + 1) && D(m) != 0) { D(m + 1) += 1; m -= 1; }
        m += 1;
    }
    for (int m = max_dn - 1; m > center;) {                                        // :61-68
        if (D(m) == 0 && D(m - 1) != 0 && D(m + 1) != 0) D(m) = D(m + 1);
        else if (D(m) == D(m - 1) && D(m) != 0) { D(m - 1) += 1; m += 1; }
        m -= 1;
    }
}

}  // namespace hm

using namespace hm;

extern "C" size_t hm_noise_profile_workspace_bytes(int64_t n_elems, int C) {
    (void)n_elems; (void)C;
    return 0;                  // the band lives in LDS and is flushed into the output: no workspace at this version
}

extern "C" int64_t hm_noise_profile_algorithmic_bytes(int n_frames, int64_t n_elems, int C) {
    return n_elems * (static_cast<int64_t>(n_frames) + 1) + int64_t{2} * 256 * 256 * C * 8;   // frames + mean once, profile read + written once
}

extern "C" int hm_noise_profile_update(const void* const* frames, int n_frames, const uint8_t* mean, int64_t n_elems, int C,
                                       int64_t* profiles, void* workspace, int64_t workspace_bytes, void* stream) {
    (void)workspace;
    bool empty;
    const int rc = hm_rules::check_noise_profile_update(frames, n_frames, mean, n_elems, C, profiles, workspace_bytes, empty);
    if (rc != HM_OK || empty) return rc;
    NoiseK k{};
    for (int i = 0; i < n_frames; ++i) k.frame[i] = static_cast<const uint8_t*>(frames[i]);
    k.mean = mean; k.prof = reinterpret_cast<unsigned long long*>(profiles); k.n = n_elems; k.n_frames = n_frames;
    // one workgroup per CU; more where a workgroup's counters could reach 2^32 (units per lane x 16 x frames x 1024 lanes)
    const int64_t units = (n_elems + kNoiseUnit - 1) / kNoiseUnit;
    const int64_t max_units_per_lane = ((int64_t{1} << 32) - 1) / (int64_t{kNoiseUnit} * n_frames * kNoiseBlock);
    int64_t grid = cu_count();
    const int64_t need = (units + kNoiseBlock - 1) / kNoiseBlock;
    if (need < grid) grid = need;
    if ((units + grid * kNoiseBlock - 1) / (grid * kNoiseBlock) > max_units_per_lane)
        grid = (units + max_units_per_lane * kNoiseBlock - 1) / (max_units_per_lane * kNoiseBlock);
    if (grid > 0x7fffffff) return HM_EUNSUPPORTED;                            // this build's own: the launch grid's limit
    const dim3 g(static_cast<unsigned>(grid)), b(kNoiseBlock);
    switch (C) {
        case 1: hipLaunchKernelGGL(k_noise_profile<1>, g, b, 0, as_stream(stream), k); break;
        case 2: hipLaunchKernelGGL(k_noise_profile<2>, g, b, 0, as_stream(stream), k); break;
        case 3: hipLaunchKernelGGL(k_noise_profile<3>, g, b, 0, as_stream(stream), k); break;
        default: hipLaunchKernelGGL(k_noise_profile<4>, g, b, 0, as_stream(stream), k); break;
    }
    return launch_status();
}

extern "C" int hm_noise_profile_std(const int64_t* profiles, int C, const double* edges, double* out_std, void* stream) {
    const int rc = hm_rules::check_noise_profile_std(profiles, C, edges, out_std);
    if (rc != HM_OK) return rc;
    const int waves = 256 * C;
    hipLaunchKernelGGL(k_noise_std, dim3((waves + 3) / 4), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const long long*>(profiles), C, edges, out_std);
    return launch_status();
}

extern "C" int hm_noise_profile_clean_edges(int64_t* profiles, int C, void* stream) {
    const int rc = hm_rules::check_noise_profile_clean_edges(profiles, C);
    if (rc != HM_OK) return rc;
    hipLaunchKernelGGL(k_noise_clean_edges, dim3((256 * C + 63) / 64), dim3(64), 0, as_stream(stream),
                       reinterpret_cast<long long*>(profiles), C);
    return launch_status();
}
