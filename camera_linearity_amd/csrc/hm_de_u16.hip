// hm_de_u16.hip - one generation of the ICRF-calibration differential evolution (hm_de.hip; the algorithm is specified in
// include/hdrmerge.h) for uint16 DN stacks of 9- to 16-bit cameras (gfx950): candidate rows of R = 2^bit_depth entries.
//
//   k_de_trial_u16           256 lanes. Lanes j < P form trial component j and its physical parameter - hm_de.hip's own text
//                            (hm_de_trial_component_body.h), so `trial` is the bits hm_de_generation writes from the same state.
//                            Lane 255 forms `last`, the unshifted row R - 1, with the row expression itself and publishes it through
//                            LDS. Then the workgroup walks segments of 256 DNs, U segments per trip: lane l forms DNs
//                            256 (s + u) + l, u < U (U independent loads per PCA component in flight, not one dependent trip per
//                            segment), shifts, stores (8 bytes per lane, coalesced) and tests them against their left neighbours -
//                            from the wave (__shfl_up), across the four wave borders through LDS (two buffers by trip parity: one
//                            barrier per trip), across segment borders from the previous segment's lane 255 (the same LDS entry;
//                            across trips a carried register). Verdicts are OR-ed in a register; one ballot per wave at the end.
//                            Up to 13 bits: grid = S, one workgroup walks the whole row and writes the byte valid[i].
//                            From 14 bits: grid = (S, slabs), 8 or 16 slabs of one or two trips. Every slab recomputes `last` and the
//                            row left of its first DN with the same expression (so also the trial components: the slabs of a member
//                            store the same `trial` values) and writes one verdict byte to the start of the workspace;
//   k_de_verdict_u16         (slab form only) one lane per member: valid[i] from its slab bytes - no atomics - before the energy
//                            stage, next in the stream, reads valid and reuses the workspace.
//   hm_linearity_energy_u16  the existing entry (hm_energy_u16.hip) on the S trial rows, called, with `variant` as given
//   k_de_select              hm_de.hip's, through de_select_launch: it never touches a row
//
// The contract is hm_de.hip's: all state is the caller's, nothing is allocated, nothing synchronises the host, no atomics; after the stop
// flag is set k_de_trial_u16, k_de_verdict_u16 and k_de_select return before their first store.
//
// hm_de_generation_u16_batch advances K problems of one shape and one depth by the same stages with the problem as one more grid
// dimension: k_de_trial_u16_batch, grid = (S, 1, K) or (S, slabs, K) - the walk's text, hm_de_trial_u16_body.h, included a second time
// on problem k's slices of the (K, ...) state and its seed -, k_de_verdict_u16_batch, grid = ((S + 255) / 256, K), on verdict bytes
// indexed (k, i, y); energy_u16_batch (hm_energy_u16.hip), candidates K x S, geometry and placement from the per-problem S and pixel
// count; k_de_select_batch (hm_de.hip) through de_select_batch_launch. A problem evolves to the same bits alone or in a batch, and every
// stage returns before its first store for a problem whose stop flag is set.
//
// Why two forms: with S = 128 members one workgroup per member leaves half the CUs idle, each of the others with one wave per SIMD. At 16
// bits (128 rows of 512 KiB) that walk took 179 us of a 204 us generation on a 28 x 28 x 7 stack; over (S, 16) workgroups the generation
// takes 74 us, at 14 bits 42 us instead of 65. At 12 bits the walk is 13 us and the two forms are within 1 us of each other: the one
// launch stays (DESIGN.md 4.4.3 has the measurements; 13 bits was not measured and is taken with 12).
#include "hm_common.h"
#include "hm_producer_math.h"
#include "hm_calibration_rules.h"
#include "hm_de_args.h"

namespace hm {

// U: segments of 256 DNs per trip; R / 256 is a multiple of U * gridDim.y (de_trial_u16_launch).
// SLAB: grid = (S, slabs); workgroup (i, y) walks the trips of slab y and writes its verdict to slab_bad[i * slabs + y] (k_de_verdict_u16
// combines them); else grid = S, one workgroup walks the whole row and writes valid[i] itself (slab_bad is not looked at).
template <int U, bool SLAB>
__global__ __launch_bounds__(256) void k_de_trial_u16(const DeK a, const int bits, uint8_t* const slab_bad) {
#include "hm_de_trial_u16_body.h"
}

// the slab form's verdict: one byte valid[i] from the member's slab bytes, before the energy stage reads it
__global__ __launch_bounds__(256) void k_de_verdict_u16(const DeK a, const uint8_t* const slab_bad, const int slabs) {
    if (a.status[HM_DE_STOP] != 0) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.S) return;
    int any = 0;
    for (int y = 0; y < slabs; ++y) any |= slab_bad[static_cast<int64_t>(i) * slabs + y];
    a.valid[i] = !any;
}

// problem k of a batch: its slices of the (K, ...) state arrays, with rows of R entries, and its seed; everything else is shared.
// Every offset is 64-bit: K * S * R * 8 bytes reach 32 GiB at the limits.
__device__ __forceinline__ DeK problem_of_rows(const DeK& a, const DeSeeds& sd, const int k, const int64_t R) {
    DeK r = a;
    const int64_t S = a.S, P = a.P, K = k;
    r.pop += K * S * P; r.energy += K * S; r.trial += K * S * P; r.trial_energy += K * S; r.icrf += K * S * R;
    r.valid += K * S; r.status += K * HM_DE_STATUS_WORDS; r.mean_icrf += K * R;
    r.pca += K * R * P;
    r.seed = sd.seed[k];
    return r;
}

// k_de_trial_u16 on problem blockIdx.z of a batch: grid = (S, 1, K), or (S, slabs, K) with the verdict bytes indexed (k, i, y)
template <int U, bool SLAB>
__global__ __launch_bounds__(256) void k_de_trial_u16_batch(const DeK a0, const DeSeeds sd, const int bits, uint8_t* const slab_bad0) {
    const DeK a = problem_of_rows(a0, sd, blockIdx.z, int64_t{1} << bits);
    uint8_t* const slab_bad = slab_bad0 + static_cast<int64_t>(blockIdx.z) * a0.S * gridDim.y;
#include "hm_de_trial_u16_body.h"
}

// k_de_verdict_u16 for a batch: grid = ((S + 255) / 256, K), one lane per member of problem blockIdx.y; nothing for a stopped problem
__global__ __launch_bounds__(256) void k_de_verdict_u16_batch(const DeK a, const uint8_t* const slab_bad, const int slabs) {
    const int64_t k = blockIdx.y;
    if (a.status[k * HM_DE_STATUS_WORDS + HM_DE_STOP] != 0) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.S) return;
    const int64_t m = k * a.S + i;
    int any = 0;
    for (int y = 0; y < slabs; ++y) any |= slab_bad[m * slabs + y];
    a.valid[m] = !any;
}

// The slab grid from this depth on (DESIGN.md 4.4.3 has the measurement: builds with 12 and 17 here against this one)
constexpr int kDeU16SlabMinBits = 14;
static_assert(kDeU16SlabMinBits >= 12, "a slab is at least one trip of 2048 DNs and a member gets at least two");
// S * slabs verdict bytes fit every workspace: hm_de_workspace_bytes is at least 16 S bytes (one pair, one chunk, two float64 per member).
// A batch's K * S * slabs bytes fit its workspace for the same reason: hm_de_batch_workspace_bytes is K times the single size.
constexpr int kDeU16MaxSlabs = 16;
static_assert(kDeU16MaxSlabs <= 2 * sizeof(double), "the verdict bytes of a member fit the 16 bytes that a workspace holds per member at least");

// 2 segments at 9 bits, 4 at 10: the whole row in one trip; 8 per trip from 11 bits on. From kDeU16SlabMinBits on the trips are
// dealt to up to kDeU16MaxSlabs workgroups per member (14 bits: 8 slabs of one trip, 15: 16 of one, 16: 16 of two), whose verdict bytes
// live at the start of the workspace until k_de_verdict_u16 has combined them - the energy stage, next in the stream, then overwrites it.
static int de_trial_u16_launch(const DeK& k, int bit_depth, void* workspace, hipStream_t st) {
    const dim3 block(256);
    uint8_t* const slab_bad = static_cast<uint8_t*>(workspace);
    if (bit_depth >= kDeU16SlabMinBits) {
        const int trips = (1 << bit_depth) >> 11, slabs = trips < kDeU16MaxSlabs ? trips : kDeU16MaxSlabs;
        hipLaunchKernelGGL((k_de_trial_u16<8, true>), dim3(k.S, slabs), block, 0, st, k, bit_depth, slab_bad);
        const int rc = launch_status();
        if (rc != HM_OK) return rc;
        hipLaunchKernelGGL(k_de_verdict_u16, dim3((k.S + 255) / 256), block, 0, st, k, slab_bad, slabs);
        return launch_status();
    }
    const dim3 grid(k.S);
    if (bit_depth == 9) hipLaunchKernelGGL((k_de_trial_u16<2, false>), grid, block, 0, st, k, bit_depth, slab_bad);
    else if (bit_depth == 10) hipLaunchKernelGGL((k_de_trial_u16<4, false>), grid, block, 0, st, k, bit_depth, slab_bad);
    else hipLaunchKernelGGL((k_de_trial_u16<8, false>), grid, block, 0, st, k, bit_depth, slab_bad);
    return launch_status();
}

// the same for the K problems of a batch: the same U per depth and the same slab counts, the problem in the grid's z (y for the verdict)
static int de_trial_u16_batch_launch(const DeK& k, const DeSeeds& sd, int n_problems, int bit_depth, void* workspace, hipStream_t st) {
    const dim3 block(256);
    uint8_t* const slab_bad = static_cast<uint8_t*>(workspace);
    if (bit_depth >= kDeU16SlabMinBits) {
        const int trips = (1 << bit_depth) >> 11, slabs = trips < kDeU16MaxSlabs ? trips : kDeU16MaxSlabs;
        hipLaunchKernelGGL((k_de_trial_u16_batch<8, true>), dim3(k.S, slabs, n_problems), block, 0, st, k, sd, bit_depth, slab_bad);
        const int rc = launch_status();
        if (rc != HM_OK) return rc;
        hipLaunchKernelGGL(k_de_verdict_u16_batch, dim3((k.S + 255) / 256, n_problems), block, 0, st, k, slab_bad, slabs);
        return launch_status();
    }
    const dim3 grid(k.S, 1, n_problems);
    if (bit_depth == 9) hipLaunchKernelGGL((k_de_trial_u16_batch<2, false>), grid, block, 0, st, k, sd, bit_depth, slab_bad);
    else if (bit_depth == 10) hipLaunchKernelGGL((k_de_trial_u16_batch<4, false>), grid, block, 0, st, k, sd, bit_depth, slab_bad);
    else hipLaunchKernelGGL((k_de_trial_u16_batch<8, false>), grid, block, 0, st, k, sd, bit_depth, slab_bad);
    return launch_status();
}

// hm_energy_u16.hip: the energy stage of hm_de_generation_u16_batch (K problems x S candidates per launch; see there)
int energy_u16_batch(const uint16_t* const* dn, const double* const* std, const int64_t* status, int n_problems, int pop_size,
                     const double* exposures, const double* icrf, const uint8_t* valid, int lower, int upper, int64_t n_pixels, int n_frames,
                     int bit_depth, int variant, double* out_energy, void* workspace, hipStream_t st);

}  // namespace hm

using namespace hm;

extern "C" int hm_de_generation_u16(double* population, double* energies, double* trial, double* trial_energies, double* icrf,
                                    uint8_t* valid, int64_t* status, const double* mean_icrf, const double* pca,
                                    const double* lower_limits, const double* upper_limits, const uint16_t* dn, const double* std,
                                    const double* exposures, int64_t n_pixels, int n_frames, int lower, int upper, int pop_size,
                                    int n_params, int64_t seed, int64_t max_generations, double mutation_lo, double mutation_hi,
                                    double recombination, double tol, double energy_limit, int bit_depth, int variant, void* workspace,
                                    void* stream) {
    int rc = hm_rules::check_de_generation_u16(population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca, lower_limits,
                                               upper_limits, dn, exposures, n_pixels, n_frames, lower, upper, pop_size, n_params,
                                               max_generations, mutation_lo, mutation_hi, recombination, tol, energy_limit, bit_depth, variant);
    if (rc != HM_OK) return rc;
    if (!workspace) return HM_EINVAL;                                         // this build's own: the energy stage's partial sums
    const DeK k = de_args(population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca, lower_limits, upper_limits,
                          pop_size, n_params, seed, max_generations, mutation_lo, mutation_hi, recombination, tol, energy_limit);
    rc = de_trial_u16_launch(k, bit_depth, workspace, as_stream(stream));
    if (rc != HM_OK) return rc;
    rc = hm_linearity_energy_u16(dn, std, exposures, icrf, valid, pop_size, lower, upper, 1, n_pixels, n_frames, bit_depth, variant, nullptr,
                                 trial_energies, workspace, stream);
    if (rc != HM_OK) return rc;
    return de_select_launch(k, as_stream(stream));
}

// K problems of one shape and one depth per call (include/hdrmerge.h): the three stages of hm_de_generation_u16 with the problem as one
// more grid dimension - k_de_trial_u16_batch (and k_de_verdict_u16_batch from 14 bits), energy_u16_batch (hm_energy_u16.hip),
// k_de_select_batch (hm_de.hip) - one linear chain on one stream. The workspace is hm_de_batch_workspace_bytes' (K times the single size).
extern "C" int hm_de_generation_u16_batch(int n_problems, double* population, double* energies, double* trial, double* trial_energies,
                                          double* icrf, uint8_t* valid, int64_t* status, const double* mean_icrf, const double* pca,
                                          const double* lower_limits, const double* upper_limits, const uint16_t* const* dn,
                                          const double* const* std, const int64_t* seeds, const double* exposures, int64_t n_pixels,
                                          int n_frames, int lower, int upper, int pop_size, int n_params, int64_t max_generations,
                                          double mutation_lo, double mutation_hi, double recombination, double tol, double energy_limit,
                                          int bit_depth, int variant, void* workspace, void* stream) {
    int rc = hm_rules::check_de_generation_u16_batch(n_problems, population, energies, trial, trial_energies, icrf, valid, status, mean_icrf,
                                                     pca, lower_limits, upper_limits, dn, std, seeds, exposures, n_pixels, n_frames, lower,
                                                     upper, pop_size, n_params, max_generations, mutation_lo, mutation_hi, recombination, tol,
                                                     energy_limit, bit_depth, variant);
    if (rc != HM_OK) return rc;
    if (!workspace) return HM_EINVAL;                                         // this build's own: the verdict bytes and the energy stage's partial sums
    const DeK k = de_args(population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca, lower_limits, upper_limits,
                          pop_size, n_params, 0, max_generations, mutation_lo, mutation_hi, recombination, tol, energy_limit);
    DeSeeds sd{};
    for (int i = 0; i < n_problems; ++i) sd.seed[i] = static_cast<uint64_t>(seeds[i]);
    rc = de_trial_u16_batch_launch(k, sd, n_problems, bit_depth, workspace, as_stream(stream));
    if (rc != HM_OK) return rc;
    rc = energy_u16_batch(dn, std, status, n_problems, pop_size, exposures, icrf, valid, lower, upper, n_pixels, n_frames, bit_depth, variant,
                          trial_energies, workspace, as_stream(stream));
    if (rc != HM_OK) return rc;
    return de_select_batch_launch(k, sd, n_problems, as_stream(stream));
}
