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
    __shared__ double x[HM_DE_MAX_PARAMS];
    __shared__ double last;
    __shared__ double edge[2][U][4];                                      // [trip parity][segment of the trip][wave]: lane 63's row
    __shared__ int bad[4];
    if (a.status[HM_DE_STOP] != 0) return;                                // uniform: the whole generation is a no-op
    const int i = blockIdx.x;
    const int lane = threadIdx.x, P = a.P, S = a.S;
    const int64_t g = a.status[HM_DE_GENERATION];

#include "hm_de_trial_component_body.h"
    __syncthreads();

    const int R = 1 << bits;
    if (lane == 255) {
        const int d = R - 1;
        double row = 0.0;
        for (int j = 0; j < P; ++j) row += a.pca[d * P + j] * x[j];       // PCA @ x, DN R - 1: the expression of the walk below
        row = a.mean_icrf[d] + row;
        last = row;
    }
    __syncthreads();
    const double shift = 1.0 - last;                                      // :166
    double* const out = a.icrf + static_cast<int64_t>(i) * R;             // S * R * 8 bytes reach 512 MiB
    const int w = lane >> 6;
    bool wrong = false;
    const int s_count = SLAB ? (R >> 8) / static_cast<int>(gridDim.y) : R >> 8;   // segments of this workgroup
    const int s_begin = SLAB ? static_cast<int>(blockIdx.y) * s_count : 0;
    double carry = 0.0;                                                   // the previous trip's last row (lane 255): DN d - 1 of lane 0
    if (SLAB && s_begin > 0) {                                            // a later slab's left neighbour: the same expression (d > 0: not row 0)
        const int d = (s_begin << 8) - 1;
        double row = 0.0;
        for (int j = 0; j < P; ++j) row += a.pca[d * P + j] * x[j];
        row = a.mean_icrf[d] + row;
        carry = row + shift;
    }
    for (int s = s_begin, trip = 0; s < s_begin + s_count; s += U, ++trip) {
        const int d0 = (s << 8) + lane;
        double row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) row[u] = 0.0;
#pragma unroll 4
        for (int j = 0; j < P; ++j) {
            const double xj = x[j];
#pragma unroll
            for (int u = 0; u < U; ++u) row[u] += a.pca[(d0 + (u << 8)) * P + j] * xj;
        }
        double (*e)[4] = edge[trip & 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int d = d0 + (u << 8);
            row[u] = a.mean_icrf[d] + row[u];
            row[u] += shift;
            if (d == 0) row[u] = 0.0;                                     // :167
            out[d] = row[u];
            if ((lane & 63) == 63) e[u][w] = row[u];
        }
        __syncthreads();
        // range (:173-175) and strict monotonicity (:177-179)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int d = d0 + (u << 8);
            double prev = __shfl_up(row[u], 1, 64);
            if ((lane & 63) == 0) prev = lane > 0 ? e[u][w - 1] : (u > 0 ? e[u - 1][3] : carry);
            wrong |= row[u] > 1.0 || row[u] < 0.0 || (d > 0 && !(row[u] > prev));
        }
        carry = e[U - 1][3];                                              // (this buffer is next written two trips on, behind the next barrier)
    }
    const unsigned long long any = __ballot(wrong);
    if ((lane & 63) == 0) bad[w] = any != 0ull;
    __syncthreads();
    if (lane == 0) {
        if (SLAB) slab_bad[static_cast<int64_t>(i) * gridDim.y + blockIdx.y] = (bad[0] | bad[1] | bad[2] | bad[3]) != 0;
        else a.valid[i] = !(bad[0] | bad[1] | bad[2] | bad[3]);
    }
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

// The slab grid from this depth on (DESIGN.md 4.4.3 has the measurement: builds with 12 and 17 here against this one)
constexpr int kDeU16SlabMinBits = 14;
static_assert(kDeU16SlabMinBits >= 12, "a slab is at least one trip of 2048 DNs and a member gets at least two");
constexpr int kDeU16MaxSlabs = 16;      // S * slabs verdict bytes fit every workspace: hm_de_workspace_bytes is at least 16 S bytes (one pair, one chunk)

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
