// hm_producer_rules.h - the argument rules of the producer entries (hm_welford_update, hm_welford_finalize, hm_welford_update_u16,
// hm_welford_finalize_u16, hm_noise_profile_update, hm_noise_profile_std, hm_noise_profile_clean_edges, hm_noise_moments_update_u16,
// hm_noise_moments_std, hm_kde_moments, hm_kde_evaluate),
// written once for both builds of the ABI in the manner of hm_merge_rules.h: the device build (hm_welford.hip, hm_welford_u16.hip,
// hm_noise.hip, hm_noise_u16.hip, hm_kde.hip) and the host build (csrc_host/hm_host.cpp) include this file and restate none of it. Plain C++17 on hdrmerge.h
// and <cmath>: no HIP type.
//
// Every status is here in the order hdrmerge.h gives them: an earlier rule wins over a later one broken in the same call. `empty` is set
// with HM_OK when there is nothing to do; which rules have been looked at by then differs per entry and is kept as it always was.
//
// The differences between the builds:
//   hm_kde_moments, hm_kde_evaluate   only the device build needs the workspace. It refuses a NULL one (HM_EINVAL) BEFORE the n_elems % C
//           rule (HM_ESHAPE): `need_workspace` keeps that place. The host build, which has nothing to ask of the workspace, asks for
//           `moments` at that place instead; the device build asks for it after the shape. After the shared call the device build
//           adds the size rules of its workspace (HM_EINVAL, last).
//   hm_noise_profile_update, hm_noise_moments_update_u16 (LDS placement)
//           after the shared call the device build refuses a launch grid beyond 2^31 - 1 (HM_EUNSUPPORTED).
#pragma once
#include "hdrmerge.h"
#include <cmath>
#include <cstdint>

namespace hm_rules {

constexpr int64_t kWelfordMaxCount = int64_t{1} << 40;       // the device build's division by the count assumes n << 2^53

// ---- the Welford entries: the statuses the uint8 and the uint16 entries share, written once ----------------------------------------
// hm_welford_update and hm_welford_update_u16 in their order, the uint16 entry's own rules at the places marked +:
//   1. HM_EINVAL        n_frames outside 0..HM_MAX_FRAMES, a negative count_before or n_elems, + bit_depth outside 9..16, + variant outside 0..3
//   2. HM_EUNSUPPORTED  count_before beyond kWelfordMaxCount
//   3. HM_ESHAPE        C outside 1..HM_MAX_CHANNELS;  4. HM_ESHAPE  n_elems no multiple of C
//   5. HM_OK, empty     no frames or no elements: nothing to do, no pointer has been looked at
//   6. HM_EUNSUPPORTED  + a forced variant that does not exist for the call or whose table does not fit (welford_u16_placement_applies)
//   7. HM_EINVAL        NULL frames, mean or frames[k]
//   8. HM_EALIGN        + a frame that is not 2-byte aligned
// rules 1-5 (the uint16 entry looks at its part of rule 1 before it calls this: the status is the same)
inline int welford_update_counts(int n_frames, int64_t count_before, int64_t n_elems, int C, bool& empty) {
    empty = false;
    if (n_frames < 0 || n_frames > HM_MAX_FRAMES || count_before < 0 || n_elems < 0) return HM_EINVAL;
    if (count_before > kWelfordMaxCount) return HM_EUNSUPPORTED;
    if (C < 1 || C > HM_MAX_CHANNELS) return HM_ESHAPE;
    if (n_elems % C != 0) return HM_ESHAPE;
    if (n_frames == 0 || n_elems == 0) empty = true;
    return HM_OK;
}
inline int welford_update_pointers(const void* const* frames, int n_frames, const double* mean) {      // rule 7
    if (!frames || !mean) return HM_EINVAL;
    for (int k = 0; k < n_frames; ++k)
        if (!frames[k]) return HM_EINVAL;
    return HM_OK;
}

inline int check_welford_update(const void* const* frames, int n_frames, int64_t count_before, const double* mean, int64_t n_elems, int C,
                                bool& empty) {
    const int rc = welford_update_counts(n_frames, count_before, n_elems, C, empty);
    if (rc != HM_OK || empty) return rc;
    return welford_update_pointers(frames, n_frames, mean);
}

// hm_welford_finalize, and hm_welford_finalize_u16 between its own two rules (check_welford_finalize_u16)
inline int check_welford_finalize(const double* mean, const double* m2, int64_t count, const void* out_mean, const void* out_std,
                                  int64_t n_elems, bool& empty) {
    empty = false;
    if (n_elems < 0 || count < 1) return HM_EINVAL;
    if (n_elems == 0) { empty = true; return HM_OK; }
    if ((out_mean && !mean) || (out_std && !m2)) return HM_EINVAL;
    if (out_std && count < 2) return HM_EINVAL;                               // m2 / (n - 1) needs two frames
    return HM_OK;
}

// frames of `bytes_per_dn`-byte DNs read once, the float64 state (mean, and m2 if present) read and written once
inline int64_t welford_algorithmic_bytes(int bytes_per_dn, int n_frames, bool with_m2, int64_t n_elems) {
    return n_elems * (static_cast<int64_t>(bytes_per_dn) * n_frames + (with_m2 ? 32 : 16));
}

// ---- hm_welford_update_u16 / hm_welford_finalize_u16: uint16 frames of bit_depth 9..16 ----------------------------------------------
// Where the device kernel takes a frame value f from (`variant`; the host build checks it and ignores it). 0 is the library's choice.
//   WELFORD_U16_LDS       a table in LDS: the ICRF as t[ch][dn] (8 * 2^b * C bytes), or without an ICRF the one column dn / M (8 * 2^b)
//   WELFORD_U16_COMPUTED  no table: f = (DN & M) / M evaluated in the lane. Exists only without an ICRF.
//   WELFORD_U16_GLOBAL    no copy: the ICRF gathered from global memory. Exists only with an ICRF.
enum WelfordU16Tab { WELFORD_U16_AUTO = 0, WELFORD_U16_LDS = 1, WELFORD_U16_COMPUTED = 2, WELFORD_U16_GLOBAL = 3 };

// The fit rule: the LDS table may take 128 KiB of the CU's 160 KiB (the rest is the workgroup's flag word and headroom) - with an ICRF
// C = 1 up to 14 bits, C = 2 up to 13, C = 3 and 4 up to 12 (96 / 128 KiB); without one up to 14 bits.
constexpr int64_t kWelfordU16LdsTableBytes = 128 * 1024;
inline int64_t welford_u16_table_bytes(int bit_depth, int C, bool with_icrf) { return (int64_t{8} << bit_depth) * (with_icrf ? C : 1); }
inline bool welford_u16_table_fits_lds(int bit_depth, int C, bool with_icrf) {
    return welford_u16_table_bytes(bit_depth, C, with_icrf) <= kWelfordU16LdsTableBytes;
}
// whether a forced placement exists for the call and its table fits
inline bool welford_u16_placement_applies(int place, int bit_depth, int C, bool with_icrf) {
    if (place == WELFORD_U16_LDS) return welford_u16_table_fits_lds(bit_depth, C, with_icrf);
    if (place == WELFORD_U16_COMPUTED) return !with_icrf;
    return place == WELFORD_U16_GLOBAL && with_icrf;
}
// variant = 0: the first placement that applies, in the order LDS, computed, global - LDS where the table fits, else the computed
// quotient (no ICRF) or global memory (ICRF). Measurements: DESIGN.md 4.4.7.
inline int welford_u16_default_placement(int bit_depth, int C, bool with_icrf) {
    if (welford_u16_table_fits_lds(bit_depth, C, with_icrf)) return WELFORD_U16_LDS;
    return with_icrf ? WELFORD_U16_GLOBAL : WELFORD_U16_COMPUTED;
}

// rules 1-6 of the list above, which look at no pointer: what hm_welford_update_u16_describe checks
inline int check_welford_update_u16_counts(int n_frames, int64_t count_before, int64_t n_elems, int C, bool with_icrf, int bit_depth, int variant,
                                           bool& empty) {
    empty = false;
    if (bit_depth < 9 || bit_depth > 16 || variant < 0 || variant > WELFORD_U16_GLOBAL) return HM_EINVAL;
    const int rc = welford_update_counts(n_frames, count_before, n_elems, C, empty);
    if (rc != HM_OK || empty) return rc;
    if (variant != WELFORD_U16_AUTO && !welford_u16_placement_applies(variant, bit_depth, C, with_icrf)) return HM_EUNSUPPORTED;
    return HM_OK;
}

inline int check_welford_update_u16(const void* const* frames, int n_frames, int64_t count_before, const double* icrf, const double* mean,
                                    int64_t n_elems, int C, int bit_depth, int variant, bool& empty) {
    int rc = check_welford_update_u16_counts(n_frames, count_before, n_elems, C, icrf != nullptr, bit_depth, variant, empty);
    if (rc != HM_OK || empty) return rc;
    rc = welford_update_pointers(frames, n_frames, mean);
    if (rc != HM_OK) return rc;
    for (int k = 0; k < n_frames; ++k)
        if (reinterpret_cast<uintptr_t>(frames[k]) & 1) return HM_EALIGN;
    return HM_OK;
}

// hm_welford_finalize's statuses in their order, + bit_depth outside 9..16 with the first (HM_EINVAL), + an output frame that is not 2-byte
// aligned last (HM_EALIGN)
inline int check_welford_finalize_u16(const double* mean, const double* m2, int64_t count, int bit_depth, const uint16_t* out_mean,
                                      const uint16_t* out_std, int64_t n_elems, bool& empty) {
    empty = false;
    if (bit_depth < 9 || bit_depth > 16) return HM_EINVAL;
    const int rc = check_welford_finalize(mean, m2, count, out_mean, out_std, n_elems, empty);
    if (rc != HM_OK || empty) return rc;
    if ((reinterpret_cast<uintptr_t>(out_mean) | reinterpret_cast<uintptr_t>(out_std)) & 1) return HM_EALIGN;
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

// ---- hm_noise_moments_update_u16 / hm_noise_moments_std: the per-level noise moments of uint16 frames of bit_depth 9..16 -------------
// Where the device kernel keeps the (2^b, C) triples of a launch (`variant`; the host build checks it and ignores it). 0 is the library's
// choice.
//   NOISE_MOMENTS_LDS     every workgroup privatises the whole table in LDS - per level and channel a u32 element count, an i64 sum of d and
//                         a u64 sum of d^2 (kNoiseMomentsLdsEntryBytes) - and flushes its non-zero entries once per launch
//   NOISE_MOMENTS_GLOBAL  no copy: every lane adds its triples to `moments` with 8-byte global atomics
//   NOISE_MOMENTS_WINDOW  a hashed window of kNoiseMomentsWindowSlots (level, channel) slots in LDS over the levels a workgroup meets, flushed
//                         after every pass over 8192 elements; a triple whose slot another level holds goes to the global atomics. Any depth.
enum NoiseMomentsTab { NOISE_MOMENTS_AUTO = 0, NOISE_MOMENTS_LDS = 1, NOISE_MOMENTS_GLOBAL = 2, NOISE_MOMENTS_WINDOW = 3 };
constexpr int kNoiseMomentsWindowBits = 12;
constexpr uint32_t kNoiseMomentsWindowSlots = 1u << kNoiseMomentsWindowBits;
constexpr int64_t kNoiseMomentsWindowBytes = int64_t{24} * kNoiseMomentsWindowSlots;        // u64 + i64 + u32 count + u32 key per slot: 96 KiB

// The fit rule: the LDS table may take 128 KiB of the CU's 160 KiB - C = 1 up to 12 bits, C = 2 and 3 up to 11, C = 4 up to 10.
constexpr int64_t kNoiseMomentsLdsTableBytes = 128 * 1024;
constexpr int64_t kNoiseMomentsLdsEntryBytes = 20;
inline int64_t noise_moments_table_bytes(int bit_depth, int C) { return (kNoiseMomentsLdsEntryBytes << bit_depth) * C; }
inline bool noise_moments_table_fits_lds(int bit_depth, int C) { return noise_moments_table_bytes(bit_depth, C) <= kNoiseMomentsLdsTableBytes; }
// variant = 0: LDS where the table fits, else the window. Measurements: DESIGN.md 4.4.8.
inline int noise_moments_default_placement(int bit_depth, int C) {
    return noise_moments_table_fits_lds(bit_depth, C) ? NOISE_MOMENTS_LDS : NOISE_MOMENTS_WINDOW;
}

// check_noise_profile_update's statuses in their order, the uint16 entry's own rules at the places marked +:
//   1. HM_EINVAL        n_frames outside 0..HM_MAX_FRAMES, a negative n_elems, C < 1, + bit_depth outside 9..16, + variant outside 0..3
//   2. HM_EUNSUPPORTED  C > HM_MAX_CHANNELS
//   3. HM_ESHAPE        n_elems no multiple of C
//   4. HM_EUNSUPPORTED  + a forced LDS placement whose table does not fit (noise_moments_table_fits_lds)
//   5. HM_EINVAL        NULL frames, mean, moments or frames[k]
//   6. HM_EALIGN        + a frame or a mean that is not 2-byte aligned
//   7. HM_OK, empty     no frames or no elements: nothing to do
// rules 1-4, which look at no pointer: what hm_noise_moments_update_u16_describe checks (it sets `empty` itself)
inline int check_noise_moments_update_counts(int n_frames, int64_t n_elems, int C, int bit_depth, int variant) {
    if (n_frames < 0 || n_frames > HM_MAX_FRAMES || n_elems < 0 || C < 1 || bit_depth < 9 || bit_depth > 16 || variant < 0 ||
        variant > NOISE_MOMENTS_WINDOW)
        return HM_EINVAL;
    if (C > HM_MAX_CHANNELS) return HM_EUNSUPPORTED;
    if (n_elems % C != 0) return HM_ESHAPE;
    if (variant == NOISE_MOMENTS_LDS && !noise_moments_table_fits_lds(bit_depth, C)) return HM_EUNSUPPORTED;
    return HM_OK;
}

inline int check_noise_moments_update(const void* const* frames, int n_frames, const uint16_t* mean, int64_t n_elems, int C, int bit_depth,
                                      const int64_t* moments, int variant, bool& empty) {
    empty = false;
    const int rc = check_noise_moments_update_counts(n_frames, n_elems, C, bit_depth, variant);
    if (rc != HM_OK) return rc;
    if (!frames || !mean || !moments) return HM_EINVAL;
    for (int k = 0; k < n_frames; ++k)
        if (!frames[k]) return HM_EINVAL;
    if (reinterpret_cast<uintptr_t>(mean) & 1) return HM_EALIGN;
    for (int k = 0; k < n_frames; ++k)
        if (reinterpret_cast<uintptr_t>(frames[k]) & 1) return HM_EALIGN;
    empty = n_frames == 0 || n_elems == 0;
    return HM_OK;
}

// HM_EINVAL for a NULL pointer, C < 1 or bit_depth outside 9..16, then HM_EUNSUPPORTED for C > HM_MAX_CHANNELS (check_noise_profile_std's order)
inline int check_noise_moments_std(const int64_t* moments, int C, int bit_depth, const double* out_std) {
    if (!moments || !out_std || C < 1 || bit_depth < 9 || bit_depth > 16) return HM_EINVAL;
    if (C > HM_MAX_CHANNELS) return HM_EUNSUPPORTED;
    return HM_OK;
}

// the frames and the mean read once (2 bytes per DN), the (2^b, C, 3) int64 state read and written once
inline int64_t noise_moments_algorithmic_bytes(int n_frames, int64_t n_elems, int C, int bit_depth) {
    return 2 * n_elems * (static_cast<int64_t>(n_frames) + 1) + ((int64_t{2} * 24) << bit_depth) * C;
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
