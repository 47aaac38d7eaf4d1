// hm_calibration_rules.h - the argument rules of the ICRF-calibration entries (hm_linearity_energy, hm_de_generation,
// hm_de_generation_batch), written once for both builds of the ABI in the manner of hm_merge_rules.h: the device build (hm_energy.hip,
// hm_de.hip) and the host build (csrc_host/hm_host.cpp) include this file and restate none of it. Plain C++17 on hdrmerge.h: no HIP type.
//
// Every status is here in the order hdrmerge.h gives them: an earlier rule wins over a later one broken in the same call.
//
// What each build adds after the shared call, and why that changes no call's status:
//   device  a NULL workspace is HM_EINVAL (the host build needs none). In all three entries it follows rules that are HM_EINVAL too or
//           comes last. The energy launch refuses a frame count its pixel-major kernels are not instantiated for (HM_EUNSUPPORTED).
//   host    hm_de_generation returns HM_OK at once when status[HM_DE_STOP] is set: there `status` is host memory. On the device build
//           the kernels read the flag, so it cannot be a rule of this file.
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

}  // namespace hm_rules
