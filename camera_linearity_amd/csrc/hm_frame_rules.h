// hm_frame_rules.h - the argument rules of the linearize entries (hm_linearize_u8 / hm_linearize_f64, hm_linearize_u16), written once for
// both builds of the ABI in the manner of hm_producer_rules.h: the device build (hm_linearize.hip) and the host build
// (csrc_host/hm_host.cpp) include this file and restate none of it. Plain C++17 on hdrmerge.h: no HIP type. At the end the body of the two
// weight-table entries (hm_gaussian_weight_lut_host, _lut_bits_host), host code that both builds export (hm_api.hip, hm_host.cpp).
// The other per-frame entries (hm_u8_to_unit_f64, hm_gaussian_weight_f64 / _u8: one or two rules each) state their rules in each build.
//
// Every rule stands in the order the entries apply it: an earlier rule wins over a later one broken in the same call. n == 0 is HM_OK
// at its place (after the table rules); the host build goes on to a loop of zero trips, the device caller returns then.
//
// The differences between the builds, each one line that names the build:
//   hm_linearize_u8 / _f64   only the device build has alignment rules; the host build asks for `icrf` only when n > 0 (n == 0 with a NULL
//                            table is HM_OK there, HM_EINVAL on the device); only the device build refuses C > HM_MAX_CHANNELS with a
//                            per-channel table (its LDS table).
//   hm_linearize_u16         none: both builds have its alignment rules.
#pragma once
#include "hm_rules_common.h"
#include <cmath>

namespace hm_rules {

// hm_linearize_u8 (f64in = false: `in` is the DN frame) and hm_linearize_f64 (f64in = true: `in` is the value frame)
inline int check_linearize(bool f64in, const void* in, const double* sd, const double* icrf, const double* out_val, const double* out_std,
                           int64_t n, int C, int lut_stride, Build build) {
    if (n < 0 || C < 1 || (!icrf && (build == DEVICE || n > 0)) || (n > 0 && (!in || !out_val))) return HM_EINVAL;
    if (lut_stride != 1 && lut_stride != C) return HM_EINVAL;
    if (build == DEVICE && C > HM_MAX_CHANNELS && lut_stride != 1) return HM_EUNSUPPORTED;
    return n > 0 && build == DEVICE && (!aligned8(out_val) || !aligned8(out_std) || !aligned8(sd) || (f64in && !aligned8(in))) ? HM_EALIGN : HM_OK;
}

inline int check_linearize_u16(const uint16_t* dn, const double* sd, const double* icrf, const double* out_val, const double* out_std,
                               const uint16_t* out_idx, int64_t n, int C, int lut_stride, int bit_depth) {
    if (n < 0 || C < 1 || !icrf || (n > 0 && (!dn || !out_val))) return HM_EINVAL;
    if ((lut_stride != 1 && lut_stride != C) || bit_depth < 9 || bit_depth > 16) return HM_EINVAL;
    const bool odd = ((reinterpret_cast<uintptr_t>(dn) | reinterpret_cast<uintptr_t>(out_idx)) & 1u) != 0;
    return n > 0 && (odd || !aligned8(out_val) || !aligned8(out_std) || !aligned8(sd)) ? HM_EALIGN : HM_OK;
}

// w and dw of measurand.py:615-616 on the grid v = k / (2^bit_depth - 1), evaluated with libm; bit_depth = 8 is the DN grid v = k / 255 of
// hm_gaussian_weight_lut_host
inline int gaussian_weight_lut(int bit_depth, double* w_lut, double* dw_lut) {
    if ((!w_lut && !dw_lut) || bit_depth < 8 || bit_depth > 16) return HM_EINVAL;
    const double max_dn = static_cast<double>((1 << bit_depth) - 1);
    for (int k = 0; k < (1 << bit_depth); ++k) {
        const double v = static_cast<double>(k) / max_dn;
        const double y = std::pow(M_E, -30.0 * ((v - 0.5) * (v - 0.5)));
        if (w_lut) w_lut[k] = y;
        if (dw_lut) dw_lut[k] = ((-2.0 * 30.0) * (v - 0.5)) * y;
    }
    return HM_OK;
}

}  // namespace hm_rules
