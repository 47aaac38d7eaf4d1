// hm_energy_dev.h - what the units of the ICRF-calibration energy share on the device and in their launchers: hm_energy.hip (uint8 stacks,
// single and batched) and hm_energy_u16.hip (uint16 stacks of 9 to 16 bits). Not an interface of the library: the pieces that must be ONE
// text for the two units to form a candidate's sums in the same order - the launch geometry, the chunk count, the wave reduction, the two
// Newton forms of the pixel-major kernel - and the launcher of k_energy_final, which hm_energy.hip defines and both units call.
#pragma once
#include "hm_common.h"

namespace hm {

// pixel-major variant (N <= kEnergyRegFrames): per-pair ratio t_i / t_j and its reciprocal from the host
constexpr int kEnergyRegFrames = 8;
constexpr int kEnergyRegPairs = kEnergyRegFrames * (kEnergyRegFrames - 1) / 2;
struct EnergyPairs {
    double ratio[kEnergyRegPairs];
    double inv_ratio[kEnergyRegPairs];
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// pair index p (row-major upper triangle, np.triu_indices(N, 1) order) -> (i, j)
__device__ __forceinline__ void pair_of(int p, int N, int& i, int& j) {
    int row = 0, left = p;
    while (left >= N - 1 - row) { left -= N - 1 - row; ++row; }
    i = row; j = row + 1 + left;
}

// 1 / sqrt(q) for the weights of the pixel-major kernel: the hardware estimate (about 2^-24) and ONE third-order step,
// y0 (1 + e/2 + 3 e^2 / 8) with e = 1 - q y0^2 - 8 instructions and at most 1.25 ulp (checked on 2 M operands against long-double
// references, as for the pair statistics) where the library's rsqrt() costs about twenty; q = 0 / inf keep the estimate (inf / 0).
__device__ __forceinline__ double rsqrt_third_order(double q) {
    const double y0 = __builtin_amdgcn_rsq(q);
    const double e = fma(-(q * y0), y0, 1.0);
    const double y = fma(y0, fma(0.375, e, 0.5) * e, y0);
    return __builtin_amdgcn_class(y0, 0x264) ? y0 : y;                  // -inf | -0 | +0 | +inf
}

// 1 / x for the per-(pixel, frame) reciprocals of the pixel-major kernel: the hardware estimate and ONE second-order step, r0 (1 + e + e^2)
// with e = 1 - x r0 - 4 instructions and at most 1.00 ulp (hm_moments.h: rcp_newton, checked on 2 M operands) where the IEEE division
// expansion costs eleven, two of them quarter-rate; x = 0 / inf / NaN keep the estimate (inf / 0 / NaN, the IEEE answers).
#ifndef HM_ENERGY_RCP
#define HM_ENERGY_RCP 1
#endif
__device__ __forceinline__ double rcp_second_order(double x) {
    const double r0 = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, r0, 1.0);
    const double r = fma(r0, fma(e, e, e), r0);
    return __builtin_amdgcn_class(r0, 0x264) ? r0 : r;                   // -inf | -0 | +0 | +inf
}

static int energy_chunks(int64_t P) {
    int64_t c = (P + 1023) / 1024;                  // >= 4 pixels per thread before splitting further
    if (c < 1) c = 1;
    return static_cast<int>(c > 64 ? 64 : c);
}

// pixel-major kernel when there are enough candidates (or few enough pixels) for chunks x candidates workgroups to
// fill the chip; a lone candidate on a large stack keeps the pair-major kernel's pairs x chunks workgroups.
// n_candidates is the count of ONE stack's candidates: a batch decides from its per-problem S, never from K x S.
static bool energy_pixel_major(int n_frames, int n_candidates, int64_t n_pixels) {
    return n_frames <= kEnergyRegFrames && (n_candidates >= 8 || n_pixels <= 16384);
}

static void energy_pair_ratios(EnergyPairs& pr, const double* exposures, int n_frames) {
    int p = 0;
    for (int i = 0; i < n_frames; ++i)
        for (int j = i + 1; j < n_frames; ++j, ++p) {
            pr.ratio[p] = exposures[i] / exposures[j];                       // :100
            pr.inv_ratio[p] = 1.0 / pr.ratio[p];
        }
}

// hm_energy.hip: k_energy_final on the partial sums of n_candidates candidates (one wave each) -> out_pairs (nullable), out_energy
int energy_final(const double* partial, const uint8_t* valid, int pairs, int chunks, int n_candidates, double* out_pairs,
                 double* out_energy, hipStream_t st);

// hm_energy.hip: k_energy_final_batch on the partial sums of `total` = K x pop_size candidates (one wave each; none for a problem whose
// stop flag in `status` (K, HM_DE_STATUS_WORDS) is set) -> out_energy
int energy_final_batch(const double* partial, const uint8_t* valid, int pairs, int chunks, int total, double* out_energy,
                       const int64_t* status, int pop_size, hipStream_t st);

}  // namespace hm
