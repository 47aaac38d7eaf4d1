// hm_calibration_rules.h - the argument rules of the ICRF-calibration entries (hm_linearity_energy, hm_linearity_energy_u16,
// hm_de_generation, hm_de_generation_u16, hm_de_generation_batch, hm_de_generation_u16_batch), written once for both builds of the ABI in the manner of
// hm_merge_rules.h: the device build (hm_energy.hip, hm_energy_u16.hip, hm_de.hip, hm_de_u16.hip) and the host build
// (csrc_host/hm_host.cpp) include this file and restate none of it.
// Plain C++17 on hdrmerge.h: no HIP type.
//
// Every status is here in the order hdrmerge.h gives them: an earlier rule wins over a later one broken in the same call.
//
// What each build adds after the shared call, and why that changes no call's status:
//   device  a NULL workspace is HM_EINVAL (the host build needs none). In all six entries it follows rules that are HM_EINVAL too or
//           comes last. The energy launch refuses a frame count its pixel-major kernels are not instantiated for (HM_EUNSUPPORTED).
//   host    hm_de_generation and hm_de_generation_u16 return HM_OK at once when status[HM_DE_STOP] is set: there `status` is host memory. On the device build
//           the kernels read the flag, so it cannot be a rule of this file. (The two batch entries call them per problem.)
#pragma once
#include "hdrmerge.h"
#include <cstdint>

namespace hm_rules {

constexpr int kEnergyMaxCandidates = 65535;          // the device build's energy grid: candidates are a grid dimension

// empty: n_candidates == 0 - nothing to do, and no pointer has been looked at
inline int check_linearity_energy(const uint8_t* dn, const double* exposures, const double* icrf, int n_candidates, int lower, int upper,
                                  int64_t n_pixels, int n_frames, const double* out_energy, bool& empty) {
    empty = false;
    if (n_candidates < 0 || n_pixels < 0) return HM_EINVAL;
    if (n_frames < 2 || n_frames > HM_MAX_FRAMES) return HM_ESHAPE;
    if (lower < 0 || lower > 255 || upper < 0 || upper > 255) return HM_EINVAL;
    if (n_candidates == 0) { empty = true; return HM_OK; }
    if (n_candidates > kEnergyMaxCandidates) return HM_EUNSUPPORTED;
    if (!dn || !exposures || !icrf || !out_energy) return HM_EINVAL;
    return HM_OK;
}

// hm_linearity_energy_u16: uint16 DNs of bit_depth 9..16, candidate rows of 2^bit_depth float64.
// variant 1 keeps the candidate's row in LDS. It fits where the row and the kernels' static reduction scratch - red[4][2 * 28] float64 of
// the pixel-major kernel at 8 frames, the largest - together are at most the CU's 160 KiB: 4 KiB + scratch at 9 bits, 32 KiB at 12,
// 128 KiB at 14; not at 15 bits (256 KiB) or 16 bits (512 KiB), where the row is gathered from global memory (variant 2).
constexpr int64_t kEnergyLdsBytes = 160 * 1024;
constexpr int64_t kEnergyU16ScratchBytes = 4 * 2 * 28 * 8;
inline bool energy_u16_row_fits_lds(int bit_depth) {
    return (int64_t{8} << bit_depth) + kEnergyU16ScratchBytes <= kEnergyLdsBytes;
}

// The statuses of hm_linearity_energy_u16, in this order:
//   1. HM_EINVAL       a negative count, bit_depth outside 9..16, variant outside 0..2
//   2. HM_ESHAPE       n_frames outside 2..HM_MAX_FRAMES
//   3. HM_EINVAL       lower or upper outside 0 .. 2^bit_depth - 1
//   4. HM_OK, empty    n_candidates == 0: nothing to do, and no pointer has been looked at
//   5. HM_EUNSUPPORTED more than kEnergyMaxCandidates candidates; variant 1 at a depth whose row does not fit LDS
//   6. HM_EINVAL       NULL dn, exposures, icrf or out_energy
//   7. HM_EALIGN       dn not 2-byte aligned
// rules 1-5, which look at no pointer: what hm_linearity_energy_u16_describe checks (with limits of 0)
inline int check_linearity_energy_u16_counts(int n_candidates, int lower, int upper, int64_t n_pixels, int n_frames, int bit_depth, int variant,
                                             bool& empty) {
    empty = false;
    if (n_candidates < 0 || n_pixels < 0 || bit_depth < 9 || bit_depth > 16 || variant < 0 || variant > 2) return HM_EINVAL;
    if (n_frames < 2 || n_frames > HM_MAX_FRAMES) return HM_ESHAPE;
    const int max_dn = (1 << bit_depth) - 1;
    if (lower < 0 || lower > max_dn || upper < 0 || upper > max_dn) return HM_EINVAL;
    if (n_candidates == 0) { empty = true; return HM_OK; }
    if (n_candidates > kEnergyMaxCandidates || (variant == 1 && !energy_u16_row_fits_lds(bit_depth))) return HM_EUNSUPPORTED;
    return HM_OK;
}

inline int check_linearity_energy_u16(const uint16_t* dn, const double* exposures, const double* icrf, int n_candidates, int lower, int upper,
                                      int64_t n_pixels, int n_frames, int bit_depth, int variant, const double* out_energy, bool& empty) {
    const int rc = check_linearity_energy_u16_counts(n_candidates, lower, upper, n_pixels, n_frames, bit_depth, variant, empty);
    if (rc != HM_OK || empty) return rc;
    if (!dn || !exposures || !icrf || !out_energy) return HM_EINVAL;
    if (reinterpret_cast<uintptr_t>(dn) & 1) return HM_EALIGN;
    return HM_OK;
}

// hm_de_generation (n_problems = 1, `stacks` its dn) and the part of hm_de_generation_batch both share (`stacks` its array of dn)
inline int check_de_generation(int n_problems, const double* population, const double* energies, const double* trial,
                               const double* trial_energies, const double* icrf, const uint8_t* valid, const int64_t* status,
                               const double* mean_icrf, const double* pca, const double* lower_limits, const double* upper_limits,
                               const void* stacks, const double* exposures, int64_t n_pixels, int n_frames, int lower, int upper,
                               int pop_size, int n_params, int64_t max_generations, double mutation_lo, double mutation_hi,
                               double recombination, double tol, double energy_limit) {
    if (pop_size < 4 || n_params < 1 || n_pixels < 0 || max_generations < 0) return HM_EINVAL;
    if (pop_size > HM_DE_MAX_POP || n_params > HM_DE_MAX_PARAMS) return HM_ESHAPE;
    if (n_frames < 2 || n_frames > HM_MAX_FRAMES) return HM_ESHAPE;
    if (n_problems * pop_size > kEnergyMaxCandidates) return HM_EUNSUPPORTED;        // (a batch only: pop_size <= HM_DE_MAX_POP)
    if (lower < 0 || lower > 255 || upper < 0 || upper > 255) return HM_EINVAL;
    if (!(mutation_lo >= 0.0 && mutation_lo <= mutation_hi && mutation_hi < 2.0)) return HM_EINVAL;                  // also rejects NaN
    if (!(recombination >= 0.0 && recombination <= 1.0) || !(tol >= 0.0) || energy_limit != energy_limit) return HM_EINVAL;
    if (!population || !energies || !trial || !trial_energies || !icrf || !valid || !status) return HM_EINVAL;
    if (!mean_icrf || !pca || !lower_limits || !upper_limits || !stacks || !exposures) return HM_EINVAL;
    return HM_OK;
}

// hm_de_generation_u16: hm_de_generation on a uint16 stack of bit_depth 9..16, rows of 2^bit_depth entries. The statuses, in this order:
//   1. hm_de_generation's, in its order, but for its limit rule (lower / upper are DNs of the depth here: rule 3 below) - a count, the
//      shape, the mutation / recombination / tol / energy_limit ranges, a NULL pointer
//   2. HM_EINVAL       bit_depth outside 9..16, variant outside 0..2                      } check_linearity_energy_u16_counts on
//   3. HM_EINVAL       lower or upper outside 0 .. 2^bit_depth - 1                         } pop_size candidates: what the energy
//   4. HM_EUNSUPPORTED variant 1 at a depth whose row does not fit LDS                     } stage would answer, before any launch
//   5. HM_EALIGN       dn not 2-byte aligned
inline int check_de_generation_u16(const double* population, const double* energies, const double* trial, const double* trial_energies,
                                   const double* icrf, const uint8_t* valid, const int64_t* status, const double* mean_icrf,
                                   const double* pca, const double* lower_limits, const double* upper_limits, const uint16_t* dn,
                                   const double* exposures, int64_t n_pixels, int n_frames, int lower, int upper, int pop_size,
                                   int n_params, int64_t max_generations, double mutation_lo, double mutation_hi, double recombination,
                                   double tol, double energy_limit, int bit_depth, int variant) {
    int rc = check_de_generation(1, population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca, lower_limits,
                                 upper_limits, dn, exposures, n_pixels, n_frames, 0, 0, pop_size, n_params, max_generations, mutation_lo,
                                 mutation_hi, recombination, tol, energy_limit);
    if (rc != HM_OK) return rc;
    bool empty;                                                               // (never: pop_size >= 4)
    rc = check_linearity_energy_u16_counts(pop_size, lower, upper, n_pixels, n_frames, bit_depth, variant, empty);
    if (rc != HM_OK) return rc;
    if (reinterpret_cast<uintptr_t>(dn) & 1) return HM_EALIGN;
    return HM_OK;
}

// dn, std_ and seeds are host arrays of n_problems entries in both builds: read within the validated count only
inline int check_de_generation_batch(int n_problems, const double* population, const double* energies, const double* trial,
                                     const double* trial_energies, const double* icrf, const uint8_t* valid, const int64_t* status,
                                     const double* mean_icrf, const double* pca, const double* lower_limits, const double* upper_limits,
                                     const uint8_t* const* dn, const double* const* std_, const int64_t* seeds, const double* exposures,
                                     int64_t n_pixels, int n_frames, int lower, int upper, int pop_size, int n_params,
                                     int64_t max_generations, double mutation_lo, double mutation_hi, double recombination, double tol,
                                     double energy_limit) {
    if (n_problems < 1) return HM_EINVAL;
    if (n_problems > HM_DE_MAX_PROBLEMS) return HM_ESHAPE;
    const int rc = check_de_generation(n_problems, population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca,
                                       lower_limits, upper_limits, dn, exposures, n_pixels, n_frames, lower, upper, pop_size, n_params,
                                       max_generations, mutation_lo, mutation_hi, recombination, tol, energy_limit);
    if (rc != HM_OK) return rc;
    if (!seeds) return HM_EINVAL;
    for (int k = 0; k < n_problems; ++k)
        if (!dn[k] || (std_ && !std_[k])) return HM_EINVAL;                   // stds for all problems or for none
    return HM_OK;
}

// hm_de_generation_u16_batch: n_problems problems on uint16 stacks of one shape and one bit_depth. The statuses, in this order:
//   1. hm_de_generation_batch's, in its order, but for its limit rule (lower / upper are DNs of the depth here): n_problems, the counts,
//      the shape, n_problems * pop_size, the mutation / recombination / tol / energy_limit ranges, a NULL pointer, a NULL seeds array, a
//      NULL entry of dn or std
//   2. hm_de_generation_u16's rules 2-4 (check_linearity_energy_u16_counts on pop_size candidates): HM_EINVAL for bit_depth outside
//      9..16, variant outside 0..2 or a limit outside 0 .. 2^bit_depth - 1; HM_EUNSUPPORTED for variant 1 where the row does not fit LDS
//   3. HM_EALIGN       a dn[k] that is not 2-byte aligned
// (the stack pointers are only compared with NULL and looked at for alignment: the batch rule takes them as the 8-bit entry's type)
inline int check_de_generation_u16_batch(int n_problems, const double* population, const double* energies, const double* trial,
                                         const double* trial_energies, const double* icrf, const uint8_t* valid, const int64_t* status,
                                         const double* mean_icrf, const double* pca, const double* lower_limits, const double* upper_limits,
                                         const uint16_t* const* dn, const double* const* std_, const int64_t* seeds, const double* exposures,
                                         int64_t n_pixels, int n_frames, int lower, int upper, int pop_size, int n_params,
                                         int64_t max_generations, double mutation_lo, double mutation_hi, double recombination, double tol,
                                         double energy_limit, int bit_depth, int variant) {
    int rc = check_de_generation_batch(n_problems, population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca,
                                       lower_limits, upper_limits, reinterpret_cast<const uint8_t* const*>(dn), std_, seeds, exposures, n_pixels,
                                       n_frames, 0, 0, pop_size, n_params, max_generations, mutation_lo, mutation_hi, recombination, tol,
                                       energy_limit);
    if (rc != HM_OK) return rc;
    bool empty;                                                               // (never: pop_size >= 4)
    rc = check_linearity_energy_u16_counts(pop_size, lower, upper, n_pixels, n_frames, bit_depth, variant, empty);
    if (rc != HM_OK) return rc;
    for (int k = 0; k < n_problems; ++k)
        if (reinterpret_cast<uintptr_t>(dn[k]) & 1) return HM_EALIGN;
    return HM_OK;
}

}  // namespace hm_rules
