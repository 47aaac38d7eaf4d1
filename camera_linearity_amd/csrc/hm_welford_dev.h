// hm_welford_dev.h - what the Welford units (hm_welford.hip: uint8 frames, hm_welford_u16.hip: uint16 frames of 9 to 16 bits) share on the
// device besides the included texts (hm_welford_lane_body.h, _fold_body.h, _finalize_body.h): the fast division's range argument, its
// predicates and constants.
//
// The fast division. delta / n must carry the bits of NumPy's IEEE division, but the divisor is the same for every element of a frame, so
// the correctly rounded reciprocal r = RN(1 / n) comes from the host per frame and the quotient is
//     q0 = RN(delta * r);   e = delta - q0 * n  (one FMA, exact);   q = RN(q0 + e * r)  (one FMA)
// which is the correctly rounded delta / n whenever r = RN(1 / n) and nothing underflows (Markstein's final division step; Brisebarre,
// Muller, Raina, IEEE TC 53(8) 2004, "division when the divisor is known in advance"). 3 dependent ops instead of the ~14-instruction IEEE
// sequence (FP64 VALU: 4 cycles per wave op).
// The range condition is checked, not assumed - once per element and launch, not per frame (round 4: the per-frame test was 2 of the 13.8
// VALU instructions of an element-frame in a kernel that is FP64-VALU bound): the fast path needs every non-zero delta >= 2^-900.
// With table entries that are 0 or in [2^-500, 2^500] (!welford_entry_odd: checked while a table is built, or on every value gathered
// where nobody sees the whole table), an incoming mean that is 0 or in [2^-540, 2^500] (welford_mean_ok) and |m2| <= 2^900 (welford_m2_ok),
// both checked at load, and n <= 2^40 (hm_rules::kWelfordMaxCount, checked on the host), every later mean is 0 or >= 2^-632 in magnitude:
// m' = m (1 - 1/n) + f/n can lose 52 bits to ONE cancellation (two doubles >= 2^-541 differ by >= 2^-593 when they differ), after which
// a non-zero f/n >= 2^-540 dwarfs it and a run of f = 0 shrinks it by n0/n >= 2^-40 at most - so a non-zero delta = f - m is >= 2^-684.
// A lane whose state or table is outside those ranges (or not finite) redoes its elements with the full division (welford_exact,
// welford_u16_exact); the state in memory is still the launch's input then.
#pragma once
#include "hm_common.h"
#include "hm_producer_math.h"
#include <type_traits>

namespace hm {

typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kWelfordGroup = 8;             // frames whose loads / table gathers are issued together

constexpr double kWelfordEntryMax = 0x1p500, kWelfordEntryMin = 0x1p-500;     // a non-zero table entry, and the incoming mean's upper end
constexpr double kWelfordMeanMin = 0x1p-540, kWelfordM2Max = 0x1p900;

__device__ __forceinline__ bool welford_entry_odd(double v) {       // non-finite, huge or tiny
    return !(fabs(v) <= kWelfordEntryMax) || (v != 0.0 && fabs(v) < kWelfordEntryMin);
}
__device__ __forceinline__ bool welford_mean_ok(double x) {
    const double ax = fabs(x);
    return x == 0.0 || (ax >= kWelfordMeanMin && ax <= kWelfordEntryMax);
}
__device__ __forceinline__ bool welford_m2_ok(double q) { return fabs(q) <= kWelfordM2Max; }

}  // namespace hm
