// hm_de.hip - one generation of the ICRF-calibration differential evolution on the device (gfx950): the solver loop of
// calibration(), modules/ICRF_calibration_exposure.py:288-369 (SciPy's DifferentialEvolutionSolver, 'currenttobest1bin',
// deferred updating), restated with counter-based random numbers - the algorithm is specified in include/hdrmerge.h.
//
//   k_de_trial    grid = S members, 256 lanes: lanes j < P form the trial component j (mutation, binomial crossover, out-of-range
//                 redraw) and its physical parameter; then lane d forms DN d of the candidate ICRF (mean + PCA x, shift, ICRF[0] = 0)
//                 and the range / monotonicity verdict is one ballot per wave, combined over the four waves in LDS
//   hm_linearity_energy   the existing energy launcher (hm_energy.hip) on the S trial rows, unchanged
//   k_de_select   ONE workgroup: deferred selection, then best index / mean / std by fixed-order LDS trees, the stop flag, and - as the
//                 last store of the generation - the generation counter
//
// All state is the caller's: nothing is allocated, nothing synchronises the host, no float atomics. The generation counter and the
// stop flag live in the status block on the device, so the same recorded launches can be replayed (hipGraph); after the stop flag is
// set k_de_trial and k_de_select return before their first store (the energy kernels re-evaluate the unchanged trial rows to the same
// bits), so the state no longer moves however many generations follow.
//
// hm_de_generation_batch advances K problems of one shape by the same three stages: k_de_trial_batch, grid = (S, K);
// energy_batch() (hm_energy.hip), candidates K x S, geometry from the per-problem S; k_de_select_batch, grid = K. The kernel
// bodies are the single-problem ones (k_de_trial's a shared function, k_de_select's the same text included a second time,
// hm_de_select_body.h) applied to problem k's slices of the (K, ...) state and to its seed, so a problem evolves to the same bits alone or in a batch; every stage, the energy kernels included, returns for a problem whose stop flag is set.
//
// hm_de_u16.hip (hm_de_generation_u16 and hm_de_generation_u16_batch: rows of 2^bit_depth entries) shares three things with this unit: DeK,
// DeSeeds and de_args (hm_de_args.h), the trial component text (hm_de_trial_component_body.h, included below: its `trial` is this unit's
// bit for bit) and k_de_select / k_de_select_batch, which it launches through de_select_launch / de_select_batch_launch.
#include "hm_common.h"
#include "hm_producer_math.h"
#include "hm_calibration_rules.h"
#include "hm_de_args.h"

namespace hm {

// hm_energy.hip: the energy stage of hm_de_generation_batch (K problems x S candidates per launch; see there)
int energy_batch(const uint8_t* const* dn, const double* const* std, const int64_t* status, int n_problems, int pop_size,
                 const double* exposures, const double* icrf, const uint8_t* valid, int lower, int upper, int64_t n_pixels,
                 int n_frames, double* out_energy, void* workspace, hipStream_t st);

// problem k of a batch: its slices of the (K, ...) state arrays and its seed; everything else is shared
__device__ __forceinline__ DeK problem_of(const DeK& a, const DeSeeds& sd, const int k) {
    DeK r = a;
    const int64_t S = a.S, P = a.P;
    r.pop += k * S * P; r.energy += k * S; r.trial += k * S * P; r.trial_energy += k * S; r.icrf += k * S * 256;
    r.valid += k * S; r.status += static_cast<int64_t>(k) * HM_DE_STATUS_WORDS; r.mean_icrf += static_cast<int64_t>(k) * 256;
    r.pca += k * 256 * P;
    r.seed = sd.seed[k];
    return r;
}

// (i: the member)
__device__ __forceinline__ void de_trial_body(const DeK& a, const int i) {
    __shared__ double x[HM_DE_MAX_PARAMS];
    __shared__ double last;
    __shared__ int bad[4];
    if (a.status[HM_DE_STOP] != 0) return;                                // uniform: the whole generation is a no-op
    const int lane = threadIdx.x, P = a.P, S = a.S;
    const int64_t g = a.status[HM_DE_GENERATION];

#include "hm_de_trial_component_body.h"
    __syncthreads();

    double row = 0.0;
    for (int j = 0; j < P; ++j) row += a.pca[lane * P + j] * x[j];        // PCA @ x, DN `lane`
    row = a.mean_icrf[lane] + row;
    if (lane == 255) last = row;
    __syncthreads();
    row += 1.0 - last;                                                    // :166
    if (lane == 0) row = 0.0;                                             // :167
    a.icrf[static_cast<int64_t>(i) * 256 + lane] = row;

    // range (:173-175) and strict monotonicity (:177-179): the left neighbour from the wave, or from the previous wave through LDS
    __shared__ double edge[4];
    if ((lane & 63) == 63) edge[lane >> 6] = row;
    __syncthreads();
    double prev = __shfl_up(row, 1, 64);
    if ((lane & 63) == 0 && lane > 0) prev = edge[(lane >> 6) - 1];
    const bool wrong = row > 1.0 || row < 0.0 || (lane > 0 && !(row > prev));
    const unsigned long long any = __ballot(wrong);
    if ((lane & 63) == 0) bad[lane >> 6] = any != 0ull;
    __syncthreads();
    if (lane == 0) a.valid[i] = !(bad[0] | bad[1] | bad[2] | bad[3]);
}

__global__ __launch_bounds__(256) void k_de_trial(const DeK a) { de_trial_body(a, blockIdx.x); }

__global__ __launch_bounds__(256) void k_de_trial_batch(const DeK a, const DeSeeds sd) {
    de_trial_body(problem_of(a, sd, blockIdx.y), blockIdx.x);
}

// fixed-order tree over n (a power of two <= HM_DE_MAX_POP) LDS entries; the result is in v[0]
__device__ __forceinline__ void tree_sum(double* v, int n) {
    for (int s = n >> 1; s > 0; s >>= 1) {
        for (int t = threadIdx.x; t < s; t += blockDim.x) v[t] += v[t + s];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_de_select(const DeK a) {
#include "hm_de_select_body.h"
}

__device__ __forceinline__ void de_select_body(const DeK& a) {
#include "hm_de_select_body.h"
}

__global__ __launch_bounds__(256) void k_de_select_batch(const DeK a, const DeSeeds sd) { de_select_body(problem_of(a, sd, blockIdx.x)); }

// (hm_de_args.h) the select stage of one problem, for this unit's hm_de_generation and for hm_de_u16.hip
int de_select_launch(const DeK& k, hipStream_t st) {
    hipLaunchKernelGGL(k_de_select, dim3(1), dim3(256), 0, st, k);
    return launch_status();
}

// (hm_de_args.h) the select stage of a batch, for this unit's hm_de_generation_batch and for hm_de_u16.hip
int de_select_batch_launch(const DeK& k, const DeSeeds& sd, int n_problems, hipStream_t st) {
    hipLaunchKernelGGL(k_de_select_batch, dim3(n_problems), dim3(256), 0, st, k, sd);
    return launch_status();
}

}  // namespace hm

using namespace hm;

extern "C" size_t hm_de_workspace_bytes(int64_t n_pixels, int n_frames, int pop_size) {
    if (pop_size < 4 || pop_size > HM_DE_MAX_POP) return 0;
    return hm_linearity_energy_workspace_bytes(n_pixels, n_frames, pop_size);
}

extern "C" int hm_de_generation(double* population, double* energies, double* trial, double* trial_energies, double* icrf,
                                uint8_t* valid, int64_t* status, const double* mean_icrf, const double* pca,
                                const double* lower_limits, const double* upper_limits, const uint8_t* dn, const double* std,
                                const double* exposures, int64_t n_pixels, int n_frames, int lower, int upper, int pop_size,
                                int n_params, int64_t seed, int64_t max_generations, double mutation_lo, double mutation_hi,
                                double recombination, double tol, double energy_limit, void* workspace, void* stream) {
    int rc = hm_rules::check_de_generation(1, population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca, lower_limits,
                                           upper_limits, dn, exposures, n_pixels, n_frames, lower, upper, pop_size, n_params, max_generations,
                                           mutation_lo, mutation_hi, recombination, tol, energy_limit);
    if (rc != HM_OK) return rc;
    if (!workspace) return HM_EINVAL;                                         // this build's own: the energy stage's partial sums
    const DeK k = de_args(population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca, lower_limits, upper_limits,
                          pop_size, n_params, seed, max_generations, mutation_lo, mutation_hi, recombination, tol, energy_limit);
    hipLaunchKernelGGL(k_de_trial, dim3(pop_size), dim3(256), 0, as_stream(stream), k);
    rc = launch_status();
    if (rc != HM_OK) return rc;
    rc = hm_linearity_energy(dn, std, exposures, icrf, valid, pop_size, lower, upper, 1, n_pixels, n_frames, nullptr,
                             trial_energies, workspace, stream);
    if (rc != HM_OK) return rc;
    return de_select_launch(k, as_stream(stream));
}

static bool de_batch_shape_ok(int pop_size, int n_problems) {
    return pop_size >= 4 && pop_size <= HM_DE_MAX_POP && n_problems >= 1 && n_problems <= HM_DE_MAX_PROBLEMS &&
           n_problems * pop_size <= 65535;
}

extern "C" size_t hm_de_batch_workspace_bytes(int64_t n_pixels, int n_frames, int pop_size, int n_problems) {
    if (!de_batch_shape_ok(pop_size, n_problems)) return 0;
    return hm_linearity_energy_workspace_bytes(n_pixels, n_frames, pop_size) * static_cast<size_t>(n_problems);
}

extern "C" int hm_de_generation_batch(int n_problems, double* population, double* energies, double* trial, double* trial_energies,
                                      double* icrf, uint8_t* valid, int64_t* status, const double* mean_icrf, const double* pca,
                                      const double* lower_limits, const double* upper_limits, const uint8_t* const* dn,
                                      const double* const* std, const int64_t* seeds, const double* exposures, int64_t n_pixels,
                                      int n_frames, int lower, int upper, int pop_size, int n_params, int64_t max_generations,
                                      double mutation_lo, double mutation_hi, double recombination, double tol, double energy_limit,
                                      void* workspace, void* stream) {
    int rc = hm_rules::check_de_generation_batch(n_problems, population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca,
                                                 lower_limits, upper_limits, dn, std, seeds, exposures, n_pixels, n_frames, lower, upper,
                                                 pop_size, n_params, max_generations, mutation_lo, mutation_hi, recombination, tol,
                                                 energy_limit);
    if (rc != HM_OK) return rc;
    if (!workspace) return HM_EINVAL;                                         // this build's own: the energy stage's partial sums
    const DeK k = de_args(population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca, lower_limits, upper_limits,
                          pop_size, n_params, 0, max_generations, mutation_lo, mutation_hi, recombination, tol, energy_limit);
    DeSeeds sd{};
    for (int i = 0; i < n_problems; ++i) sd.seed[i] = static_cast<uint64_t>(seeds[i]);
    hipLaunchKernelGGL(k_de_trial_batch, dim3(pop_size, n_problems), dim3(256), 0, as_stream(stream), k, sd);
    rc = launch_status();
    if (rc != HM_OK) return rc;
    rc = energy_batch(dn, std, status, n_problems, pop_size, exposures, icrf, valid, lower, upper, n_pixels, n_frames, trial_energies,
                      workspace, as_stream(stream));
    if (rc != HM_OK) return rc;
    return de_select_batch_launch(k, sd, n_problems, as_stream(stream));
}
