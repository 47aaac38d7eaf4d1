// hm_energy.hip - the ICRF-calibration energy function on the device (gfx950), for a whole population of
// candidate ICRFs per launch: _energy_function + analyze_linearity,
// modules/ICRF_calibration_exposure.py:66-145,148-201.
//
//   per candidate b (a 256-entry ICRF of one channel), frame pair i < j, pixel p:
//       v_i = ICRF_b[dn[p, i]], NaN if v_i < ICRF_b[lower] or v_i > ICRF_b[upper]        (:96-97,:186-194)
//       ratio = t_i / t_j                                                                  (:100)
//       scaled = v_j * ratio                                                               (:111)
//       d = v_i - scaled;  relative: d /= scaled;  a = |d|                                (:114-120)
//       with std:  sigma = sqrt((s_i / scaled)^2 + ((v_i * s_j) / (ratio * v_j^2))^2)     (:127)
//                  (absolute: sqrt(s_i^2 + (ratio * s_j)^2)                                :129)
//                  w = 1 / sigma where a is finite and sigma != 0, else excluded          (:133-134)
//                  result[i, j] = sum(a * w) / sum(w), NaN when sum(w) == 0               (general_functions.py:164-174)
//       without:   result[i, j] = nanmean(a)                                              (:138)
//   energy_b = nanmean over the pairs, +inf if that is NaN                                (:196-198)
//
// The stack is the reference's (X, Y, N) layout flattened to (P, N): a pixel's N samples are adjacent.
// Two launch geometries (chosen in hm_linearity_energy): pair-major, grid = (pixel chunks, pairs, candidates), every
// workgroup reduces one pair of one candidate over one pixel chunk (any N; a lone candidate still fills the chip
// with pairs x chunks workgroups); pixel-major for N <= 8, grid = (pixel chunks, candidates), all pairs of a pixel
// from registers (see k_energy_pixel). The reference evaluates one candidate at a time on the host. The sums are
// formed in a fixed order (lane-strided, shuffle tree, chunk order), so results are reproducible run to run;
// they differ from NumPy's pairwise summation in the last bits (tests: 1e-12 relative).
//
// Batched forms (k_energy_pixel_batch, k_energy_partial_batch, k_energy_final_batch; energy_batch() below) serve
// hm_de_generation_batch: the candidate dimension spans K problems x S candidates, candidate b belongs to problem b / S and
// reads THAT problem's stack, and the workgroups of a problem whose stop flag is set return before their first store. The
// kernel bodies are the single-stack kernels' own text, included a second time (hm_energy_pixel_body.h, hm_energy_partial_body.h;
// k_energy_final's is a shared function) and the geometry and the chunk count come from the per-problem S and pixel count
// (energy_pixel_major, energy_chunks), so a candidate's sums are formed in the same order - the same bits - whether its problem is
// evaluated alone or in a batch.
//
// uint16 stacks of 9- to 16-bit cameras: hm_energy_u16.hip, the same bodies with candidate rows of 2^bit_depth entries. What the two units
// share beside the bodies - geometry, chunk count, reductions, the launcher of k_energy_final - is in hm_energy_dev.h.
#include "hm_energy_dev.h"
#include "hm_calibration_rules.h"

namespace hm {

// where the kernel bodies keep the candidate's row (hm_energy_pixel_body.h, hm_energy_partial_body.h): all 256 entries in static LDS, one
// per thread of the workgroup; a DN is its own index
#define HM_ENERGY_ROW_DECL __shared__ double lut[256];
#define HM_ENERGY_ROW_FILL(b) lut[threadIdx.x] = a.icrf[static_cast<int64_t>(b) * 256 + threadIdx.x]; __syncthreads();
#define HM_ENERGY_ROW(dn) lut[dn]

struct EnergyK {
    const uint8_t* dn;        // (P, N)
    const double* sd;         // (P, N) or null
    const double* icrf;       // (B, 256)
    const uint8_t* valid;     // (B) or null: 0 = candidate rejected on the host, energy preset to +inf
    double* partial;          // (B, pairs, chunks, 2)
    int64_t P;
    int32_t N, lower, upper, relative, chunks;
    double t[HM_MAX_FRAMES];
};

// the problems of a batch: the stacks travel in the kernel arguments (a recorded graph holds them by value)
struct EnergyBatch {
    const uint8_t* dn[HM_DE_MAX_PROBLEMS];   // (P, N) each
    const double* sd[HM_DE_MAX_PROBLEMS];    // (P, N) each; read only by the STD kernels
    const int64_t* status;                   // (K, HM_DE_STATUS_WORDS): the stop flags
    int32_t S;                               // candidates per problem
};

__device__ __forceinline__ bool batch_stopped(const EnergyBatch& q, int k) {
    return q.status[static_cast<int64_t>(k) * HM_DE_STATUS_WORDS + HM_DE_STOP] != 0;
}

// the arguments of problem k's candidates: the shared ones, reading that problem's stack
__device__ __forceinline__ EnergyK on_stack_of(const EnergyK& a, const EnergyBatch& q, int k) {
    EnergyK r = a;
    r.dn = q.dn[k]; r.sd = q.sd[k];
    return r;
}

template <bool STD>
__global__ __launch_bounds__(256) void k_energy_partial(const EnergyK a) {
#include "hm_energy_partial_body.h"
}

template <bool STD>
__device__ __forceinline__ void energy_partial_body(const EnergyK a) {
#include "hm_energy_partial_body.h"
}

template <bool STD>
__global__ __launch_bounds__(256) void k_energy_partial_batch(const EnergyK a, const EnergyBatch q) {
    const int k = blockIdx.z / q.S;
    if (batch_stopped(q, k)) return;                  // uniform per workgroup: a stopped problem costs no pixel work
    energy_partial_body<STD>(on_stack_of(a, q, k));
}

// Pixel-major evaluation for N <= 8 frames: a thread owns pixels, reads their N samples (and stds) once, maps them
// through the candidate's ICRF and evaluates ALL N(N-1)/2 pairs from registers, with the per-pair sums in registers
// too (2 x 28 float64 at most). Against the pair-major kernel above this removes the N-fold re-reads of the stack
// (27 GB of HBM traffic per 75-candidate launch on a 1024 x 1024 x 7 stack, profiles/r01e_producers_pmc.json) and
// the four IEEE divisions + square root per pair-pixel: 1 / v_j is formed once per (pixel, frame), 1 / (v_j ratio) is
// a product, and the weight 1 / sigma is one reciprocal square root. Those products differ from the reference's
// quotients by an ulp or two per term (tests: 1e-12 relative on the pair results).
template <int N, bool STD>
__global__ __launch_bounds__(256) void k_energy_pixel(const EnergyK a, const EnergyPairs pr) {
#include "hm_energy_pixel_body.h"
}

template <int N, bool STD>
__device__ __forceinline__ void energy_pixel_body(const EnergyK a, const EnergyPairs pr) {
#include "hm_energy_pixel_body.h"
}

template <int N, bool STD>
__global__ __launch_bounds__(256) void k_energy_pixel_batch(const EnergyK a, const EnergyPairs pr, const EnergyBatch q) {
    const int k = blockIdx.y / q.S;
    if (batch_stopped(q, k)) return;
    energy_pixel_body<N, STD>(on_stack_of(a, q, k), pr);
}

// one wave per candidate: pair results (chunks summed in order) and the NaN-ignoring mean over pairs
__device__ __forceinline__ void energy_final_body(const double* __restrict__ partial, const uint8_t* __restrict__ valid,
                                                  int pairs, int chunks, double* __restrict__ out_pairs,
                                                  double* __restrict__ out_energy, const int b) {
    const int lane = threadIdx.x;
    const bool ok = !valid || valid[b];
    double sum = 0.0, cnt = 0.0;
    for (int p = lane; p < pairs; p += 64) {
        const double* q = partial + (static_cast<int64_t>(b) * pairs + p) * chunks * 2;
        double num = 0.0, den = 0.0;
        for (int c = 0; c < chunks; ++c) { num += q[2 * c]; den += q[2 * c + 1]; }
        const double r = ok ? num / den : __builtin_nan("");           // 0 / 0 = NaN: no contributing pixel
        if (out_pairs) out_pairs[static_cast<int64_t>(b) * pairs + p] = r;
        if (r == r) { sum += r; cnt += 1.0; }
    }
    sum = wave_sum(sum); cnt = wave_sum(cnt);
    if (lane == 0) {
        const double e = sum / cnt;
        out_energy[b] = (ok && e == e) ? e : __builtin_inf();
    }
}

__global__ __launch_bounds__(64) void k_energy_final(const double* __restrict__ partial, const uint8_t* __restrict__ valid,
                                                     int pairs, int chunks, double* __restrict__ out_pairs,
                                                     double* __restrict__ out_energy) {
    energy_final_body(partial, valid, pairs, chunks, out_pairs, out_energy, blockIdx.x);
}

// the batch: one wave per candidate of every problem, none for a stopped problem (its partials were not rewritten)
__global__ __launch_bounds__(64) void k_energy_final_batch(const double* __restrict__ partial, const uint8_t* __restrict__ valid,
                                                           int pairs, int chunks, double* __restrict__ out_energy,
                                                           const int64_t* __restrict__ status, int S) {
    const int b = blockIdx.x;
    if (status[static_cast<int64_t>(b / S) * HM_DE_STATUS_WORDS + HM_DE_STOP] != 0) return;
    energy_final_body(partial, valid, pairs, chunks, nullptr, out_energy, b);
}

int energy_final(const double* partial, const uint8_t* valid, int pairs, int chunks, int n_candidates, double* out_pairs,
                 double* out_energy, hipStream_t st) {
    hipLaunchKernelGGL(k_energy_final, dim3(n_candidates), dim3(64), 0, st, partial, valid, pairs, chunks, out_pairs, out_energy);
    return launch_status();
}

// (hm_energy_dev.h) k_energy_final_batch on the partial sums of `total` = K x S candidates, for energy_batch below and for hm_energy_u16.hip
int energy_final_batch(const double* partial, const uint8_t* valid, int pairs, int chunks, int total, double* out_energy,
                       const int64_t* status, int pop_size, hipStream_t st) {
    hipLaunchKernelGGL(k_energy_final_batch, dim3(total), dim3(64), 0, st, partial, valid, pairs, chunks, out_energy, status, pop_size);
    return launch_status();
}

// the kernel arguments of one launch (validated by the caller); a batch passes no stack here: on_stack_of() gives each problem its own
static EnergyK energy_args(const uint8_t* dn, const double* std, const double* exposures, const double* icrf, const uint8_t* valid,
                           int lower, int upper, int relative, int64_t n_pixels, int n_frames, void* workspace) {
    EnergyK k{};
    k.dn = dn; k.sd = std; k.icrf = icrf; k.valid = valid; k.partial = static_cast<double*>(workspace);
    k.P = n_pixels; k.N = n_frames; k.lower = lower; k.upper = upper; k.relative = relative;
    k.chunks = energy_chunks(n_pixels);
    for (int i = 0; i < n_frames; ++i) k.t[i] = exposures[i];
    return k;
}

// hm_de_generation_batch's energy stage (arguments validated there): the relative energies of the S candidates of each of
// K problems, rows k S .. k S + S - 1 of icrf / valid / out_energy, on problem k's stack; workspace as K single launches.
int energy_batch(const uint8_t* const* dn, const double* const* std, const int64_t* status, int n_problems, int pop_size,
                 const double* exposures, const double* icrf, const uint8_t* valid, int lower, int upper, int64_t n_pixels,
                 int n_frames, double* out_energy, void* workspace, hipStream_t st) {
    const int pairs = n_frames * (n_frames - 1) / 2, total = n_problems * pop_size;
    const EnergyK k = energy_args(nullptr, nullptr, exposures, icrf, valid, lower, upper, 1, n_pixels, n_frames, workspace);
    EnergyBatch q{};
    for (int i = 0; i < n_problems; ++i) { q.dn[i] = dn[i]; q.sd[i] = std ? std[i] : nullptr; }
    q.status = status; q.S = pop_size;
    if (energy_pixel_major(n_frames, pop_size, n_pixels)) {
        EnergyPairs pr{};
        energy_pair_ratios(pr, exposures, n_frames);
        const dim3 grid(k.chunks, total);
#define HM_EPX(n) case n: if (std) hipLaunchKernelGGL((k_energy_pixel_batch<n, true>), grid, dim3(256), 0, st, k, pr, q); \
                          else hipLaunchKernelGGL((k_energy_pixel_batch<n, false>), grid, dim3(256), 0, st, k, pr, q); break;
        switch (n_frames) { HM_EPX(2) HM_EPX(3) HM_EPX(4) HM_EPX(5) HM_EPX(6) HM_EPX(7) HM_EPX(8) default: return HM_EUNSUPPORTED; }
#undef HM_EPX
    } else {
        const dim3 grid(k.chunks, pairs, total);
        if (std) hipLaunchKernelGGL(k_energy_partial_batch<true>, grid, dim3(256), 0, st, k, q);
        else     hipLaunchKernelGGL(k_energy_partial_batch<false>, grid, dim3(256), 0, st, k, q);
    }
    int rc = launch_status();
    if (rc != HM_OK) return rc;
    return energy_final_batch(static_cast<const double*>(workspace), valid, pairs, k.chunks, total, out_energy, status, pop_size, st);
}

}  // namespace hm

using namespace hm;

extern "C" size_t hm_linearity_energy_workspace_bytes(int64_t n_pixels, int n_frames, int n_candidates) {
    if (n_pixels < 0 || n_frames < 2 || n_candidates < 1) return 0;
    const int64_t pairs = static_cast<int64_t>(n_frames) * (n_frames - 1) / 2;
    return static_cast<size_t>(n_candidates) * pairs * energy_chunks(n_pixels) * 2 * sizeof(double);
}

extern "C" int hm_linearity_energy(const uint8_t* dn, const double* std, const double* exposures, const double* icrf,
                                   const uint8_t* valid, int n_candidates, int lower, int upper, int use_relative,
                                   int64_t n_pixels, int n_frames, double* out_pairs, double* out_energy,
                                   void* workspace, void* stream) {
    bool empty;
    const int rc0 = hm_rules::check_linearity_energy(dn, exposures, icrf, n_candidates, lower, upper, n_pixels, n_frames, out_energy, empty);
    if (rc0 != HM_OK || empty) return rc0;
    if (!workspace) return HM_EINVAL;                                         // this build's own: the partial sums live there
    const int pairs = n_frames * (n_frames - 1) / 2;
    const EnergyK k = energy_args(dn, std, exposures, icrf, valid, lower, upper, use_relative ? 1 : 0, n_pixels, n_frames, workspace);
    if (energy_pixel_major(n_frames, n_candidates, n_pixels)) {
        EnergyPairs pr{};
        energy_pair_ratios(pr, exposures, n_frames);
        const dim3 grid(k.chunks, n_candidates);
#define HM_EPX(n) case n: if (std) hipLaunchKernelGGL((k_energy_pixel<n, true>), grid, dim3(256), 0, as_stream(stream), k, pr); \
                          else hipLaunchKernelGGL((k_energy_pixel<n, false>), grid, dim3(256), 0, as_stream(stream), k, pr); break;
        switch (n_frames) { HM_EPX(2) HM_EPX(3) HM_EPX(4) HM_EPX(5) HM_EPX(6) HM_EPX(7) HM_EPX(8) default: return HM_EUNSUPPORTED; }
#undef HM_EPX
    } else {
        const dim3 grid(k.chunks, pairs, n_candidates);
        if (std) hipLaunchKernelGGL(k_energy_partial<true>, grid, dim3(256), 0, as_stream(stream), k);
        else     hipLaunchKernelGGL(k_energy_partial<false>, grid, dim3(256), 0, as_stream(stream), k);
    }
    int rc = launch_status();
    if (rc != HM_OK) return rc;
    return energy_final(static_cast<const double*>(workspace), valid, pairs, k.chunks, n_candidates, out_pairs, out_energy, as_stream(stream));
}
