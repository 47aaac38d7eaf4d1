// hm_energy_u16.hip - the ICRF-calibration energy function (hm_energy.hip; the arithmetic is described there) on uint16 DN stacks of 9 to
// 16 bits: candidate ICRFs of n = 2^bit_depth rows, a DN's index DN & (n - 1) before every table access (hm_merge_u16's convention).
//
// The kernels are hm_energy.hip's own text - hm_energy_pixel_body.h for N <= 8 frames, hm_energy_partial_body.h for any N - with the same
// geometry (energy_pixel_major, energy_chunks, 256-thread workgroups, lane-strided pixel walk) and the same reduction (wave_sum, red[4],
// k_energy_final): an 8-bit problem embedded at depth b (DN << (b - 8), the 256 entries at rows k << (b - 8)) gives hm_linearity_energy's bits.
// What differs is where a candidate's row of 8 * 2^b bytes lives while a workgroup reads it (LDS template parameter):
//   lut=lds     dynamic LDS, filled by the workgroup's 256 threads in a strided loop: up to 14 bits (128 KiB + the reduction scratch;
//               hm_rules::energy_u16_row_fits_lds). At 13 and 14 bits two workgroups / one workgroup per CU: slower than the gather.
//   lut=global  gathered from the (n_candidates, n) table through L1 and L2: every depth, the only form at 15 and 16 bits.
// variant 0 takes energy_u16_default_lds() (measured: DESIGN.md 4.4.3), 1 and 2 force a placement; both placements read the same values
// in the same order, so they agree bit for bit.
//
// Batched forms (k_energy_pixel_u16_batch, k_energy_partial_u16_batch; energy_u16_batch() below) serve hm_de_generation_u16_batch as
// hm_energy.hip's serve hm_de_generation_batch: the candidate dimension spans K problems x S candidates, candidate b belongs to problem
// b / S and reads THAT problem's stack, the workgroups of a stopped problem return before the row fill, and the geometry, the chunk count
// and the placement come from ONE problem's S and pixel count - the same sums in the same order, alone or in a batch. The final
// reduction is hm_energy.hip's k_energy_final_batch.
#include "hm_energy_dev.h"
#include "hm_calibration_rules.h"
#include <cstdio>
#include <mutex>
#include <string>

namespace hm {

struct EnergyU16K {
    const uint16_t* dn;       // (P, N)
    const double* sd;         // (P, N) or null
    const double* icrf;       // (B, n)
    const uint8_t* valid;     // (B) or null: 0 = candidate rejected on the host, energy preset to +inf
    double* partial;          // (B, pairs, chunks, 2)
    int64_t P;
    int32_t N, lower, upper, relative, chunks;
    int32_t n;                // rows of a candidate: 2^bit_depth
    uint32_t mask;            // n - 1
    double t[HM_MAX_FRAMES];
};

// the candidate's row for the kernel bodies: `grow` is the row in the global table, row_lds its copy where LDS says so
#define HM_ENERGY_ROW_DECL extern __shared__ double row_lds[]; const double* grow;
#define HM_ENERGY_ROW_FILL(b) \
    grow = a.icrf + static_cast<int64_t>(b) * a.n; \
    if (LDS) { \
        for (int r = threadIdx.x; r < a.n; r += 256) row_lds[r] = grow[r]; \
        __syncthreads(); \
    }
#define HM_ENERGY_ROW(dn) (LDS ? row_lds[(dn) & a.mask] : grow[(dn) & a.mask])

template <bool STD, bool LDS>
__global__ __launch_bounds__(256) void k_energy_partial_u16(const EnergyU16K a) {
#include "hm_energy_partial_body.h"
}

template <int N, bool STD, bool LDS>
__global__ __launch_bounds__(256) void k_energy_pixel_u16(const EnergyU16K a, const EnergyPairs pr) {
#include "hm_energy_pixel_body.h"
}

// The problems of a batch (hm_de_generation_u16_batch; hm_energy.hip's EnergyBatch with uint16 stacks): the stacks travel in the kernel
// arguments, so a recorded graph holds them by value. Candidate b belongs to problem b / S and reads THAT problem's stack.
struct EnergyU16Batch {
    const uint16_t* dn[HM_DE_MAX_PROBLEMS];  // (P, N) each
    const double* sd[HM_DE_MAX_PROBLEMS];    // (P, N) each; read only by the STD kernels
    const int64_t* status;                   // (K, HM_DE_STATUS_WORDS): the stop flags
    int32_t S;                               // candidates per problem
};
static_assert(sizeof(EnergyU16K) + sizeof(EnergyPairs) + sizeof(EnergyU16Batch) <= 4096, "the kernel arguments of a batched launch stay within 4096 bytes");

__device__ __forceinline__ bool batch_stopped(const EnergyU16Batch& q, int k) {
    return q.status[static_cast<int64_t>(k) * HM_DE_STATUS_WORDS + HM_DE_STOP] != 0;
}

// The batched kernels: the same two body texts once more, reading the stack of the candidate's problem (HM_ENERGY_DN / HM_ENERGY_SD name
// it; the arguments' own dn / sd are not looked at), after the stop test - a stopped problem's workgroups return before the row fill and
// before their first store (uniform per workgroup).
// Order matters: the single kernels above must stay above. Their inclusion of the body headers is what defined the two names as a.dn /
// a.sd; moved below this point they would name stack_dn / stack_sd, which they do not declare (a compile error, not a wrong result).
#undef HM_ENERGY_DN
#undef HM_ENERGY_SD
#define HM_ENERGY_DN stack_dn
#define HM_ENERGY_SD stack_sd

template <bool STD, bool LDS>
__global__ __launch_bounds__(256) void k_energy_partial_u16_batch(const EnergyU16K a, const EnergyU16Batch batch) {
    const int problem = blockIdx.z / batch.S;
    if (batch_stopped(batch, problem)) return;
    const uint16_t* const stack_dn = batch.dn[problem];
    const double* const stack_sd = batch.sd[problem];
#include "hm_energy_partial_body.h"
}

template <int N, bool STD, bool LDS>
__global__ __launch_bounds__(256) void k_energy_pixel_u16_batch(const EnergyU16K a, const EnergyPairs pr, const EnergyU16Batch batch) {
    const int problem = blockIdx.y / batch.S;
    if (batch_stopped(batch, problem)) return;
    const uint16_t* const stack_dn = batch.dn[problem];
    const double* const stack_sd = batch.sd[problem];
#include "hm_energy_pixel_body.h"
}

#undef HM_ENERGY_DN
#undef HM_ENERGY_SD

#undef HM_ENERGY_ROW_DECL
#undef HM_ENERGY_ROW_FILL
#undef HM_ENERGY_ROW

// More dynamic LDS than a kernel gets by default: every lut=lds instantiation is given the CU's 160 KiB less the static reduction scratch
// (the runtime refuses a dynamic limit that does not fit beside a kernel's static LDS), once per process, on the first launch of any of
// them (host-side, no stream work: the entry stays capturable after its first call).
static_assert(hm_rules::kEnergyLdsBytes == kMaxLds, "the fit rule is stated for this device's LDS");
static int energy_u16_lds_limit() {
    static std::once_flag once;
    static int status = HM_OK;
    std::call_once(once, [] {
#define HM_EPX(n) reinterpret_cast<const void*>(&k_energy_pixel_u16<n, false, true>), reinterpret_cast<const void*>(&k_energy_pixel_u16<n, true, true>), \
                  reinterpret_cast<const void*>(&k_energy_pixel_u16_batch<n, false, true>), reinterpret_cast<const void*>(&k_energy_pixel_u16_batch<n, true, true>),
        const void* fns[] = {HM_EPX(2) HM_EPX(3) HM_EPX(4) HM_EPX(5) HM_EPX(6) HM_EPX(7) HM_EPX(8)
                             reinterpret_cast<const void*>(&k_energy_partial_u16<false, true>),
                             reinterpret_cast<const void*>(&k_energy_partial_u16<true, true>),
                             reinterpret_cast<const void*>(&k_energy_partial_u16_batch<false, true>),
                             reinterpret_cast<const void*>(&k_energy_partial_u16_batch<true, true>)};
#undef HM_EPX
        for (const void* fn : fns)
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds - static_cast<int>(hm_rules::kEnergyU16ScratchBytes)) != hipSuccess) { (void)hipGetLastError(); status = HM_ELAUNCH; }
    });
    return status;
}

// The library's choice of the row's placement (variant = 0), from tools/bench_energy_u16.py (the table is in DESIGN.md 4.4.3): a copy in
// LDS pays where every entry of the row is read often enough to return the fill that each workgroup repeats - measured: stacks of 7 M
// samples at 10 and 12 bits, in both geometries; not stacks of 0.46 M samples or fewer - and only up to 12 bits: at 14 bits one workgroup
// per CU loses to the gather at every size measured (13 bits: not measured, taken with 14).
static bool energy_u16_default_lds(int bit_depth, int64_t n_pixels, int n_frames) {
    return bit_depth <= 12 && n_pixels * n_frames >= (int64_t{1024} << bit_depth);
}

// The launches of hm_linearity_energy_u16 on validated arguments - or, with `describe`, the name of the pixel kernel they would start
// and no launch (so the description cannot drift from the dispatch; dn, std, icrf, out_* and workspace are then not looked at).
static int energy_u16_run(const uint16_t* dn, const double* std, const double* exposures, const double* icrf, const uint8_t* valid,
                          int n_candidates, int lower, int upper, int relative, int64_t n_pixels, int n_frames, int bit_depth, int variant,
                          bool with_std, double* out_pairs, double* out_energy, void* workspace, hipStream_t st, std::string* describe) {
    const int pairs = n_frames * (n_frames - 1) / 2;
    const bool lds = variant == 1 || (variant == 0 && energy_u16_default_lds(bit_depth, n_pixels, n_frames));
    const bool pixel_major = energy_pixel_major(n_frames, n_candidates, n_pixels);
    if (describe) {
        char buf[96];
        if (pixel_major) snprintf(buf, sizeof buf, "k_energy_pixel_u16<N=%d,std=%d,lut=%s,bits=%d>", n_frames, with_std, lds ? "lds" : "global", bit_depth);
        else snprintf(buf, sizeof buf, "k_energy_partial_u16<std=%d,lut=%s,bits=%d>(N=%d)", with_std, lds ? "lds" : "global", bit_depth, n_frames);
        *describe = buf;
        return HM_OK;
    }
    EnergyU16K k{};
    k.dn = dn; k.sd = std; k.icrf = icrf; k.valid = valid; k.partial = static_cast<double*>(workspace);
    k.P = n_pixels; k.N = n_frames; k.lower = lower; k.upper = upper; k.relative = relative;
    k.chunks = energy_chunks(n_pixels);
    k.n = 1 << bit_depth; k.mask = static_cast<uint32_t>(k.n - 1);
    for (int i = 0; i < n_frames; ++i) k.t[i] = exposures[i];
    unsigned lds_bytes = 0;
    if (lds) {
        const int rc = energy_u16_lds_limit();
        if (rc != HM_OK) return rc;
        lds_bytes = static_cast<unsigned>(sizeof(double)) << bit_depth;
    }
    if (pixel_major) {
        EnergyPairs pr{};
        energy_pair_ratios(pr, exposures, n_frames);
        const dim3 grid(k.chunks, n_candidates);
#define HM_EPX_L(n, S) if (lds) hipLaunchKernelGGL((k_energy_pixel_u16<n, S, true>), grid, dim3(256), lds_bytes, st, k, pr); \
                       else hipLaunchKernelGGL((k_energy_pixel_u16<n, S, false>), grid, dim3(256), 0, st, k, pr);
#define HM_EPX(n) case n: if (with_std) { HM_EPX_L(n, true) } else { HM_EPX_L(n, false) } break;
        switch (n_frames) { HM_EPX(2) HM_EPX(3) HM_EPX(4) HM_EPX(5) HM_EPX(6) HM_EPX(7) HM_EPX(8) default: return HM_EUNSUPPORTED; }
#undef HM_EPX
#undef HM_EPX_L
    } else {
        const dim3 grid(k.chunks, pairs, n_candidates);
        if (with_std) { if (lds) hipLaunchKernelGGL((k_energy_partial_u16<true, true>), grid, dim3(256), lds_bytes, st, k);
                        else hipLaunchKernelGGL((k_energy_partial_u16<true, false>), grid, dim3(256), 0, st, k); }
        else          { if (lds) hipLaunchKernelGGL((k_energy_partial_u16<false, true>), grid, dim3(256), lds_bytes, st, k);
                        else hipLaunchKernelGGL((k_energy_partial_u16<false, false>), grid, dim3(256), 0, st, k); }
    }
    const int rc = launch_status();
    if (rc != HM_OK) return rc;
    return energy_final(static_cast<const double*>(workspace), valid, pairs, k.chunks, n_candidates, out_pairs, out_energy, st);
}

// hm_de_generation_u16_batch's energy stage (arguments validated there): the relative energies of the S candidates of each of K problems,
// rows k S .. k S + S - 1 of icrf / valid / out_energy, on problem k's stack; workspace as K single launches. The geometry, the chunk
// count and the row's placement are energy_u16_run's for ONE problem - pop_size candidates on n_pixels pixels, never K x S -, so a
// candidate's sums are formed in the same order, the same bits, alone or in a batch. The final reduction is hm_energy.hip's
// k_energy_final_batch (energy_final_batch).
int energy_u16_batch(const uint16_t* const* dn, const double* const* std, const int64_t* status, int n_problems, int pop_size,
                     const double* exposures, const double* icrf, const uint8_t* valid, int lower, int upper, int64_t n_pixels, int n_frames,
                     int bit_depth, int variant, double* out_energy, void* workspace, hipStream_t st) {
    const int pairs = n_frames * (n_frames - 1) / 2, total = n_problems * pop_size;
    const bool lds = variant == 1 || (variant == 0 && energy_u16_default_lds(bit_depth, n_pixels, n_frames));
    EnergyU16K k{};
    k.icrf = icrf; k.valid = valid; k.partial = static_cast<double*>(workspace);
    k.P = n_pixels; k.N = n_frames; k.lower = lower; k.upper = upper; k.relative = 1;
    k.chunks = energy_chunks(n_pixels);
    k.n = 1 << bit_depth; k.mask = static_cast<uint32_t>(k.n - 1);
    for (int i = 0; i < n_frames; ++i) k.t[i] = exposures[i];
    EnergyU16Batch q{};
    for (int i = 0; i < n_problems; ++i) { q.dn[i] = dn[i]; q.sd[i] = std ? std[i] : nullptr; }
    q.status = status; q.S = pop_size;
    unsigned lds_bytes = 0;
    if (lds) {
        const int rc = energy_u16_lds_limit();
        if (rc != HM_OK) return rc;
        lds_bytes = static_cast<unsigned>(sizeof(double)) << bit_depth;
    }
    if (energy_pixel_major(n_frames, pop_size, n_pixels)) {
        EnergyPairs pr{};
        energy_pair_ratios(pr, exposures, n_frames);
        const dim3 grid(k.chunks, total);
#define HM_EPX_L(n, S) if (lds) hipLaunchKernelGGL((k_energy_pixel_u16_batch<n, S, true>), grid, dim3(256), lds_bytes, st, k, pr, q); \
                       else hipLaunchKernelGGL((k_energy_pixel_u16_batch<n, S, false>), grid, dim3(256), 0, st, k, pr, q);
#define HM_EPX(n) case n: if (std) { HM_EPX_L(n, true) } else { HM_EPX_L(n, false) } break;
        switch (n_frames) { HM_EPX(2) HM_EPX(3) HM_EPX(4) HM_EPX(5) HM_EPX(6) HM_EPX(7) HM_EPX(8) default: return HM_EUNSUPPORTED; }
#undef HM_EPX
#undef HM_EPX_L
    } else {
        const dim3 grid(k.chunks, pairs, total);
        if (std) { if (lds) hipLaunchKernelGGL((k_energy_partial_u16_batch<true, true>), grid, dim3(256), lds_bytes, st, k, q);
                   else hipLaunchKernelGGL((k_energy_partial_u16_batch<true, false>), grid, dim3(256), 0, st, k, q); }
        else     { if (lds) hipLaunchKernelGGL((k_energy_partial_u16_batch<false, true>), grid, dim3(256), lds_bytes, st, k, q);
                   else hipLaunchKernelGGL((k_energy_partial_u16_batch<false, false>), grid, dim3(256), 0, st, k, q); }
    }
    const int rc = launch_status();
    if (rc != HM_OK) return rc;
    return energy_final_batch(static_cast<const double*>(workspace), valid, pairs, k.chunks, total, out_energy, status, pop_size, st);
}

}  // namespace hm

using namespace hm;

extern "C" int hm_linearity_energy_u16(const uint16_t* dn, const double* std, const double* exposures, const double* icrf,
                                       const uint8_t* valid, int n_candidates, int lower, int upper, int use_relative,
                                       int64_t n_pixels, int n_frames, int bit_depth, int variant, double* out_pairs, double* out_energy,
                                       void* workspace, void* stream) {
    bool empty;
    const int rc0 = hm_rules::check_linearity_energy_u16(dn, exposures, icrf, n_candidates, lower, upper, n_pixels, n_frames, bit_depth, variant,
                                                         out_energy, empty);
    if (rc0 != HM_OK || empty) return rc0;
    if (!workspace) return HM_EINVAL;                                         // this build's own: the partial sums live there
    return energy_u16_run(dn, std, exposures, icrf, valid, n_candidates, lower, upper, use_relative ? 1 : 0, n_pixels, n_frames, bit_depth,
                          variant, std != nullptr, out_pairs, out_energy, workspace, as_stream(stream), nullptr);
}

extern "C" int hm_linearity_energy_u16_describe(int64_t n_pixels, int n_frames, int n_candidates, int with_std, int bit_depth, int variant,
                                                char* buf, int buf_len) {
    if (!buf || buf_len < 1) return HM_EINVAL;
    buf[0] = '\0';
    bool empty;
    const int rc0 = hm_rules::check_linearity_energy_u16_counts(n_candidates, 0, 0, n_pixels, n_frames, bit_depth, variant, empty);
    if (rc0 != HM_OK || empty) return rc0;
    std::string name;
    const int rc = energy_u16_run(nullptr, nullptr, nullptr, nullptr, nullptr, n_candidates, 0, 0, 1, n_pixels, n_frames, bit_depth, variant,
                                  with_std != 0, nullptr, nullptr, nullptr, nullptr, &name);
    snprintf(buf, static_cast<size_t>(buf_len), "%s", name.c_str());
    return rc;
}
