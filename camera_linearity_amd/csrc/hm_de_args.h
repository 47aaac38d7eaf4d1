// hm_de_args.h - the arguments of one differential-evolution generation as the kernels of hm_de.hip and hm_de_u16.hip take them (DeK,
// and DeSeeds for a batch), and what those two units share on the host side. Plain C++ on <cstdint>: ../csrc_host/hm_host.cpp fills a DeK too, for the trial
// component text it shares with the device kernels (hm_de_trial_component_body.h).
#pragma once
#include "hdrmerge.h"
#include <cstdint>

namespace hm {

struct DeK {
    double* pop;              // (S, P) scaled to [0, 1]
    double* energy;           // (S)
    double* trial;            // (S, P)
    double* trial_energy;     // (S)
    double* icrf;             // (S, 256); (S, 2^bit_depth) for hm_de_generation_u16
    uint8_t* valid;           // (S)
    int64_t* status;          // HM_DE_STATUS_WORDS
    const double* mean_icrf;  // (256); (2^bit_depth)
    const double* pca;        // (256, P); (2^bit_depth, P)
    const double* lo;         // (P)
    const double* hi;         // (P)
    int32_t S, P;
    uint64_t seed;
    int64_t max_generations;
    double m_lo, m_hi, cr, tol, energy_limit;
};

// the kernel arguments of a generation, as given (hm_calibration_rules.h judges them first); a batch passes no seed here: its seeds travel in DeSeeds
inline DeK de_args(double* population, double* energies, double* trial, double* trial_energies, double* icrf, uint8_t* valid,
                   int64_t* status, const double* mean_icrf, const double* pca, const double* lower_limits, const double* upper_limits,
                   int pop_size, int n_params, int64_t seed, int64_t max_generations, double mutation_lo, double mutation_hi,
                   double recombination, double tol, double energy_limit) {
    DeK k{};
    k.pop = population; k.energy = energies; k.trial = trial; k.trial_energy = trial_energies; k.icrf = icrf; k.valid = valid;
    k.status = status; k.mean_icrf = mean_icrf; k.pca = pca; k.lo = lower_limits; k.hi = upper_limits;
    k.S = pop_size; k.P = n_params; k.seed = static_cast<uint64_t>(seed); k.max_generations = max_generations;
    k.m_lo = mutation_lo; k.m_hi = mutation_hi; k.cr = recombination; k.tol = tol; k.energy_limit = energy_limit;
    return k;
}

// the seeds of a batch travel in the kernel arguments, like the stack pointers of its energy stage
struct DeSeeds {
    uint64_t seed[HM_DE_MAX_PROBLEMS];
};

#ifdef __HIPCC__
// hm_de.hip: k_de_select on one problem's state (the last stage of hm_de_generation, and of hm_de_generation_u16 in hm_de_u16.hip) -> status
int de_select_launch(const DeK& k, hipStream_t st);
// hm_de.hip: k_de_select_batch on the (K, ...) state of n_problems problems (the last stage of hm_de_generation_batch, and of
// hm_de_generation_u16_batch in hm_de_u16.hip: the selection never touches a row, so the rows' length does not matter to it) -> status
int de_select_batch_launch(const DeK& k, const DeSeeds& sd, int n_problems, hipStream_t st);
#endif

}  // namespace hm
