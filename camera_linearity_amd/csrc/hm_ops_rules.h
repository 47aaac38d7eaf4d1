// hm_ops_rules.h - the argument rules of the operator and pointwise entries (hm_binary_op, hm_unary_op, hm_pow_scalar, hm_take_axis,
// hm_apply_thresholds, hm_compute_difference, hm_interpolate and their _bcast forms), written once for both builds of the ABI in the manner
// of hm_producer_rules.h: the device build (hm_ops.hip, hm_pointwise.hip) and the host build (csrc_host/hm_host.cpp) include this file and
// restate none of it. Plain C++17 on hdrmerge.h: no HIP type. The broadcast validation is check_bcast() of hm_rules_common.h.
//
// Every rule stands in the order the entries apply it: an earlier rule wins over a later one broken in the same call. No element is
// HM_OK at its place (which rules have been looked at by then differs per entry and is kept as it always was); the host build goes on to
// loops of zero trips, the device caller returns then.
//
// The differences between the builds, each one line that names the build:
//   HM_EALIGN       only the device build has alignment rules (hm_binary_op, hm_unary_op, hm_pow_scalar, hm_apply_thresholds; the
//                   difference and interpolation entries have none in either build).
//   hm_take_axis    only the device build refuses n_indices > HM_TAKE_MAX (its kernel argument holds that many), between two HM_EINVAL rules.
#pragma once
#include "hm_rules_common.h"

namespace hm_rules {

// n: the element count of the broadcast result
inline int check_binary_op(int op, const double* x1, const double* s1, const double* x2, const double* s2, const double* out_val,
                           const double* out_std, int ndim, const int64_t* shape, const int64_t* strides1, const int64_t* strides2, Build build,
                           int64_t& n) {
    if (op < HM_OP_ADD || op > HM_OP_POW || ndim < 1 || ndim > HM_MAX_DIMS || !shape || !strides1 || !strides2) return HM_EINVAL;
    if (!x1 || !x2 || !out_val) return HM_EINVAL;
    if ((out_std != nullptr) != (s1 != nullptr || s2 != nullptr)) return HM_EINVAL;
    if (build == DEVICE && (!aligned8(x1) || !aligned8(x2) || !aligned8(out_val))) return HM_EALIGN;
    return check_bcast(ndim, shape, strides1, strides2, n) ? HM_OK : HM_EINVAL;
}

// hm_unary_op, and hm_pow_scalar: the same rules but the first (its caller passes a valid op)
inline int check_unary_op(int op, const double* x, const double* s, const double* out_val, const double* out_std, int64_t n, Build build) {
    if (op < HM_UOP_NEG || op > HM_UOP_LOG_10 || n < 0) return HM_EINVAL;
    if (n == 0) return HM_OK;
    if (!x || !out_val || ((out_std != nullptr) != (s != nullptr))) return HM_EINVAL;
    return build == DEVICE && (!aligned8(x) || !aligned8(out_val)) ? HM_EALIGN : HM_OK;
}

// room() -> the caller's array of n_indices entries, asked for only once the rules before the index loop have passed (a refused call
// allocates nothing). It receives the indices, negative ones counted from the end of the axis (NumPy's), for the caller to gather with.
template <typename Room>
inline int check_take_axis(const double* x, const double* s, const double* out_val, const double* out_std, int64_t outer, int64_t axis_len,
                           int64_t inner, const int64_t* indices, int n_indices, Build build, Room room) {
    if (!x || !out_val || !indices || outer < 0 || axis_len < 1 || inner < 1 || n_indices < 1) return HM_EINVAL;
    if (build == DEVICE && n_indices > HM_TAKE_MAX) return HM_EUNSUPPORTED;
    if ((out_std != nullptr) != (s != nullptr)) return HM_EINVAL;
    int64_t* const idx = room();
    for (int q = 0; q < n_indices; ++q) {
        int64_t v = indices[q];
        if (v < 0) v += axis_len;
        if (v < 0 || v >= axis_len) return HM_ESHAPE;           // np.take raises IndexError (mode='raise')
        idx[q] = v;
    }
    return HM_OK;
}

inline int check_apply_thresholds(const double* val, const double* sd, const double* lower, const double* upper, int64_t n, int C, Build build) {
    if (n < 0 || C < 1 || !lower || !upper) return HM_EINVAL;
    if (C > HM_THRESHOLD_MAX_CHANNELS) return HM_EUNSUPPORTED;
    if (n == 0) return HM_OK;
    if (!val) return HM_EINVAL;
    return build == DEVICE && (!aligned8(val) || !aligned8(sd)) ? HM_EALIGN : HM_OK;
}

// hm_compute_difference and hm_interpolate are their _bcast forms on ndim = 1, shape = {n}, strides = {1}, and are checked as such: the same
// rules in the same order (n < 0 is the negative extent). No difference between the builds.
inline int check_compute_difference_bcast(const double* x, const double* sx, const double* y, const double* sy, const double* out_abs,
                                          const double* out_abs_std, const double* out_rel, const double* out_rel_std, int ndim,
                                          const int64_t* shape, const int64_t* strides_x, const int64_t* strides_y, int64_t& n) {
    if (!check_bcast(ndim, shape, strides_x, strides_y, n)) return HM_EINVAL;
    if (n == 0) return HM_OK;
    if (!x || !y || !out_abs || !out_rel) return HM_EINVAL;
    return (sx || sy) != (out_abs_std != nullptr) || (sx || sy) != (out_rel_std != nullptr) ? HM_EINVAL : HM_OK;
}

inline int check_interpolate_bcast(const double* x0, const double* s0, const double* x1, const double* s1, const double* out, const double* out_std,
                                   int ndim, const int64_t* shape, const int64_t* strides0, const int64_t* strides1, int64_t& n) {
    if (!check_bcast(ndim, shape, strides0, strides1, n)) return HM_EINVAL;
    if (n == 0) return HM_OK;
    return !x0 || !x1 || !out || ((s0 || s1) != (out_std != nullptr)) ? HM_EINVAL : HM_OK;
}

}  // namespace hm_rules
