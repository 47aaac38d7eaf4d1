// hm_producer_math.h - the element formulas of the upstream producers, one text for the device units (hm_welford.hip, hm_welford_u16.hip,
// hm_noise.hip, hm_noise_u16.hip, hm_de.hip) and ../csrc_host/hm_host.cpp: the uint8 / uint16 rounding of the Welford result (round_to_dn
// picks by output type: the finalize text of both depths calls it), the edge cleaning of one noise-profile row, one level of the STD table
// from its noise moments, and the counter-based uniform draws of the differential evolution. Not the Welford fold: as a shared function it moved the device kernels (hm_welford_fold_body.h).
//
// DEVICE / HOST - the builds perform the same operations here.
#pragma once
#include "hm_math_common.h"

namespace hm {

// np.around(x).astype(uint8): round half to even, then the low byte of the 64-bit integer; NaN and |x| beyond 9.2e18 -> 0 (no
// out-of-range conversion in either build)
HM_MATH_FN uint8_t round_to_u8(double x) {
    const double r = rint(x);
    if (!(r == r)) return 0;
    if (r >= 9.2e18 || r <= -9.2e18) return 0;
    return static_cast<uint8_t>(static_cast<uint64_t>(static_cast<int64_t>(r)) & 255u);
}

// np.around(x).astype(uint16) by the same convention: the low 16 bits of the 64-bit integer, so round_to_u16(x) & 255 == round_to_u8(x)
HM_MATH_FN uint16_t round_to_u16(double x) {
    const double r = rint(x);
    if (!(r == r)) return 0;
    if (r >= 9.2e18 || r <= -9.2e18) return 0;
    return static_cast<uint16_t>(static_cast<uint64_t>(static_cast<int64_t>(r)) & 65535u);
}

// the one of the two for a DN of type Out (uint8_t, uint16_t): the Welford finalize of both depths is one text
template <typename Out>
HM_MATH_FN Out round_to_dn(double x) {
    if constexpr (sizeof(Out) == 1) return round_to_u8(x);
    else return round_to_u16(x);
}

// Python's x // 2 on a 64-bit integer
HM_MATH_FN int64_t floordiv2(int64_t x) { return x >= 0 ? x / 2 : -((-x + 1) / 2); }

// clean_data_edges, modules/video_processing.py:12-74, on one (row, channel) of a noise profile: the reference's four integer passes
// centred at `center`, in order, in place. D(m) is a reference to bin m of the row, m in 0..255.
template <typename Row>
HM_MATH_FN void clean_edges_row(const Row& D, int center) {
    const int min_dn = 0, max_dn = 255;
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

// One level of the per-DN STD table from its noise moments (hm_noise_moments_std): n frame-elements with S1 = sum d and S2 = sum d^2,
// d = frame DN - mean DN. _calculate_STD's sqrt(sum((x - mean)^2 h) / n) on the DN grid x = f / M is sqrt(n S2 - S1^2) / n / M: the numerator
// N = n S2 - S1^2 is formed exactly in 128-bit integers (up to 126 bits), converted half by half (no 128-bit conversion exists on the
// device), and the rest is FP64 - at most five roundings. n = 0 gives 0 / 0 = NaN (deviation L); moments no data set can have (N < 0): NaN.
HM_MATH_FN double noise_moments_level_std(int64_t n, int64_t s1, int64_t s2, double max_dn) {
    const uint64_t a1 = s1 < 0 ? uint64_t{0} - static_cast<uint64_t>(s1) : static_cast<uint64_t>(s1);
    const unsigned __int128 ns2 = static_cast<unsigned __int128>(static_cast<uint64_t>(n)) * static_cast<uint64_t>(s2);
    const unsigned __int128 sq = static_cast<unsigned __int128>(a1) * a1;
    if (n < 0 || ns2 < sq) return NAN;
    const unsigned __int128 num = ns2 - sq;
    const uint64_t hi = static_cast<uint64_t>(num >> 64), lo = static_cast<uint64_t>(num);
    const double x = hi ? static_cast<double>(hi) * 0x1.0p64 + static_cast<double>(lo) : static_cast<double>(lo);
    return sqrt(x) / static_cast<double>(n) / max_dn;
}

// the splitmix64 step, and draw k of member i of a generation's key as a double in [0, 1) (53 bits)
HM_MATH_FN uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
HM_MATH_FN double de_uniform(uint64_t key, int i, int k) {
    const uint64_t r = mix64(key + (static_cast<uint64_t>(i + 1) << 20) + static_cast<uint64_t>(k));
    return static_cast<double>(r >> 11) * 0x1.0p-53;
}

}  // namespace hm
