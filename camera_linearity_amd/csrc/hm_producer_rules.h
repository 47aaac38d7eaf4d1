// hm_producer_rules.h - the argument rules of the producer entries (hm_welford_update, hm_welford_finalize, hm_noise_profile_update,
// hm_noise_profile_std, hm_noise_profile_clean_edges, hm_kde_moments, hm_kde_evaluate), written once for both builds of the ABI in the
// manner of hm_merge_rules.h: the device build (hm_welford.hip, hm_noise.hip, hm_kde.hip) and the host build (csrc_host/hm_host.cpp)
// include this file and restate none of it. Plain C++17 on hdrmerge.h and <cmath>: no HIP type.
//
// Every status is here in the order hdrmerge.h gives them: an earlier rule wins over a later one broken in the same call. `empty` is set
// with HM_OK when there is nothing to do; which rules have been looked at by then differs per entry and is kept as it always was.
//
// The differences between the builds:
//   hm_kde_moments, hm_kde_evaluate   only the device build needs the workspace. It refuses a NULL one (HM_EINVAL) BEFORE the n_elems % C
//           rule (HM_ESHAPE): `need_workspace` keeps that place. The host build, which has nothing to ask of the workspace, asks for
//           `moments` at that place instead; the device build asks for it after the shape. After the shared call the device build
//           adds the size rules of its workspace (HM_EINVAL, last).
//   hm_noise_profile_update           after the shared call the device build refuses a launch grid beyond 2^31 - 1 (HM_EUNSUPPORTED).
#pragma once
#include "hdrmerge.h"
#include <cmath>
#include <cstdint>

namespace hm_rules {

constexpr int64_t kWelfordMaxCount = int64_t{1} << 40;       // the device build's division by the count assumes n << 2^53

inline int check_welford_update(const void* const* frames, int n_frames, int64_t count_before, const double* mean, int64_t n_elems, int C,
                                bool& empty) {
    empty = false;
    if (n_frames < 0 || n_frames > HM_MAX_FRAMES || count_before < 0 || n_elems < 0) return HM_EINVAL;
    if (count_before > kWelfordMaxCount) return HM_EUNSUPPORTED;
    if (C < 1 || C > HM_MAX_CHANNELS) return HM_ESHAPE;
    if (n_elems % C != 0) return HM_ESHAPE;
    if (n_frames == 0 || n_elems == 0) { empty = true; return HM_OK; }
    if (!frames || !mean) return HM_EINVAL;
    for (int k = 0; k < n_frames; ++k)
        if (!frames[k]) return HM_EINVAL;
    return HM_OK;
}

inline int check_welford_finalize(const double* mean, const double* m2, int64_t count, const uint8_t* out_mean, const uint8_t* out_std,
                                  int64_t n_elems, bool& empty) {
    empty = false;
    if (n_elems < 0 || count < 1) return HM_EINVAL;
    if (n_elems == 0) { empty = true; return HM_OK; }
    if ((out_mean && !mean) || (out_std && !m2)) return HM_EINVAL;
    if (out_std && count < 2) return HM_EINVAL;                               // m2 / (n - 1) needs two frames
    return HM_OK;
}

inline int check_noise_profile_update(const void* const* frames, int n_frames, const uint8_t* mean, int64_t n_elems, int C,
                                      const int64_t* profiles, int64_t workspace_bytes, bool& empty) {
    empty = false;
    if (n_frames < 0 || n_frames > HM_MAX_FRAMES || n_elems < 0 || C < 1 || workspace_bytes < 0) return HM_EINVAL;
    if (C > HM_MAX_CHANNELS) return HM_EUNSUPPORTED;
    if (n_elems % C != 0) return HM_ESHAPE;
    if (!frames || !mean || !profiles) return HM_EINVAL;
    for (int k = 0; k < n_frames; ++k)
        if (!frames[k]) return HM_EINVAL;
    empty = n_frames == 0 || n_elems == 0;
    return HM_OK;
}

inline int check_noise_profile_std(const int64_t* profiles, int C, const double* edges, const double* out_std) {
    if (!profiles || !edges || !out_std || C < 1) return HM_EINVAL;
    if (C > HM_MAX_CHANNELS) return HM_EUNSUPPORTED;
    return HM_OK;
}

inline int check_noise_profile_clean_edges(const int64_t* profiles, int C) {
    if (!profiles || C < 1) return HM_EINVAL;
    if (C > HM_MAX_CHANNELS) return HM_EUNSUPPORTED;
    return HM_OK;
}

inline int check_kde_moments(const double* val, int64_t n_elems, int C, int channel, const double* moments, const void* workspace,
                             int64_t workspace_bytes, bool need_workspace) {
    if (!val || n_elems < 0 || C < 1 || channel < 0 || channel >= C || workspace_bytes < 0) return HM_EINVAL;
    if (need_workspace ? !workspace : !moments) return HM_EINVAL;
    if (n_elems % C != 0) return HM_ESHAPE;
    if (!moments) return HM_EINVAL;
    return HM_OK;
}

// empty: m == 0 - nothing to do; grid and out have not been looked at
inline int check_kde_evaluate(const double* val, int64_t n_elems, int C, int channel, double h, double scale, const double* grid, int m,
                              const double* out, const void* workspace, int64_t workspace_bytes, bool need_workspace, bool& empty) {
    empty = false;
    if (!val || n_elems < 0 || C < 1 || channel < 0 || channel >= C || workspace_bytes < 0 || (need_workspace && !workspace)) return HM_EINVAL;
    if (n_elems % C != 0) return HM_ESHAPE;
    if (m < 0 || !(h > 0.0) || !std::isfinite(h) || !std::isfinite(scale)) return HM_EINVAL;
    if (m == 0) { empty = true; return HM_OK; }
    if (!grid || !out) return HM_EINVAL;
    return HM_OK;
}

}  // namespace hm_rules
