// hm_rules_common.h - what the rule headers of namespace hm_rules (hm_frame_rules.h, hm_ops_rules.h, hm_pairs_rules.h) and the statistics
// entries of both builds share: the build a check is asked for, the 8-byte alignment predicate, the element count of a dense block and the
// broadcast validation. Plain C++17 on hdrmerge.h: no HIP type; the device units and csrc_host/hm_host.cpp include it.
#pragma once
#include "hdrmerge.h"
#include <cstdint>
#include <initializer_list>

namespace hm_rules {

// A check takes the build it runs in. A rule that only one build applies is one line that names the build, where that build applies it.
enum Build { DEVICE, HOST };

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }       // NULL is aligned

// the element count of a dense block of the given extents, or -1 when an extent is < 1 or the product is above 2^48 (absurd arguments
// must come back as HM_EINVAL / 0, not as an integer overflow inside the launch arithmetic)
inline int64_t dense_elems(std::initializer_list<int64_t> dims) {
    int64_t n = 1;
    for (int64_t d : dims)
        if (d < 1 || __builtin_mul_overflow(n, d, &n) || n > (int64_t{1} << 48)) return -1;
    return n;
}

// The broadcast arguments of hm_binary_op and the _bcast entries: ndim in 1..HM_MAX_DIMS, three arrays of ndim entries, no negative extent
// or stride. n = the product of the extents: 0 when one of them is 0, and a product beyond int64 is refused like a negative extent.
inline bool check_bcast(int ndim, const int64_t* shape, const int64_t* st1, const int64_t* st2, int64_t& n) {
    if (ndim < 1 || ndim > HM_MAX_DIMS || !shape || !st1 || !st2) return false;
    bool none = false, beyond = false;
    n = 1;
    for (int d = 0; d < ndim; ++d) {
        if (shape[d] < 0 || st1[d] < 0 || st2[d] < 0) return false;
        none = none || shape[d] == 0;
        beyond = beyond || __builtin_mul_overflow(n, shape[d], &n);
    }
    if (none) n = 0;
    return none || !beyond;
}

}  // namespace hm_rules
