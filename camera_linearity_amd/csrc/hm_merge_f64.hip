// hm_merge_f64.hip - merge_f64_val / merge_f64_std: the fused merge's streaming kernels for float64 frames (gfx950), with launch_f64.
// The kernel map of the whole merge is in hm_merge.hip.
#include "hm_merge_host.h"

namespace hm {

// ------------------------------------------------------------------------------------------------
// merge_f64_val / merge_f64_std (body: merge_f64_body): float64 frames (the reference's 64-bit mode, image_set.py:225 / frames saved by save_64bit) with the
// streaming decomposition of merge_u8_loop: lane l owns elements 2l, 2l+1 of a 128-element group, every frame / std /
// output access is one 16-byte load or store per lane (1 KB contiguous per wave instruction). The weight is evaluated
// analytically (measurand.py:615-616) and the LUT index is computed (round-half-even, wrap, :503), exactly as
// merge_generic does; val-only needs one pass (S and the numerator accumulate together), std needs S first and
// re-evaluates the weights in its second pass. Stacks of up to 8 frames keep the frame VALUES in registers between
// the passes; larger ones re-read them (not the weights: with exp() stubbed out the kernel is 1.5 % faster, it is
// bound by memory traffic, and the re-read misses the caches). merge_generic evaluated exp() twice per
// element-frame even for val-only and moved 8-byte pieces: 1 307 -> see docs/DESIGN_history_r01_r02.md section 8 for the numbers.
// ------------------------------------------------------------------------------------------------

#ifndef HM_F64_KEEP_W
#define HM_F64_KEEP_W 1      // float64-frame std kernel: keep pass 1's weights in registers for pass 2 (N <= 8): one exp() per
#endif                       // element-frame instead of two; with 3 waves/SIMD 1 385 -> 1 296 us on 7 x 4096 x 4096 x 3 (profiles/r02c_ab_f64std.log)

constexpr int kF64Chunk = 4;
constexpr int kF64Keep = 8;        // std mode: stacks up to this size keep their frame values in registers between the passes

template <int C, bool STD, bool FLAT, bool SUMW, int OUT>
__device__ __forceinline__ void merge_f64_body(const MergeK& a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    reset_hot_counters(a);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lane2 = lane * 2u, lane16 = lane * 16u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr uint32_t WPB = 4;
    const uint32_t n_groups = static_cast<uint32_t>(a.n_elems / kSub);
    const uint32_t gstride = gridDim.x * WPB;
    const int N = a.n_frames;
    double2* t_gd = reinterpret_cast<double2*>(lds);                              // {g, d} per (dn, c)
    for (int i = threadIdx.x; i < 256 * C; i += 256) t_gd[i] = double2{a.icrf[i], STD ? a.icrf_diff[i] : 0.0};
    double2* t_flat = reinterpret_cast<double2*>(lds + 16 * 256 * C);
    if constexpr (FLAT) {
        for (int i = threadIdx.x; i < 256; i += 256) {
            const double F = static_cast<double>(i) / 255.0;
            t_flat[i] = double2{F, 1.0 / (F * F)};
        }
    }
    __syncthreads();
    auto ld2 = [&](const double* base) -> f64x2 {
        return __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(reinterpret_cast<const char*>(base) + lane16));
    };

#ifndef HM_F64_PREFETCH
#define HM_F64_PREFETCH 0    // std mode, N <= kF64Keep: the next group's frame values loaded (second register set) before the current group's exp()s.
                             // Round 3, measured and left off: the kernel sits at its 3-waves/SIMD register budget (166 VGPRs) and the second set spills
                             // (1 890 us against 1 305 us on 7 x 4096 x 4096 x 3 + std); at 2 waves/SIMD 1 565 us, without the kept weights 1 456 us,
                             // that at 4 waves/SIMD 1 745 us (profiles/r03_ab_f64std_prefetch.log). As with the uint8 std kernels, more loads in
                             // flight per wave do not help a kernel that already covers bandwidth x latency across its waves.
#endif
    constexpr bool PRE = STD && HM_F64_PREFETCH;
    const bool keep_regs = STD && N <= kF64Keep;                                  // wave-uniform
    f64x2 vpre[PRE ? kF64Keep : 1];
    if constexpr (PRE) {
        const uint32_t g0 = blockIdx.x * WPB + wave;
        if (keep_regs && g0 < n_groups) {
#pragma unroll
            for (int i = 0; i < kF64Keep; ++i)
                if (i < N) vpre[i] = ld2(static_cast<const double*>(a.frame[i]) + a.in_off + static_cast<int64_t>(g0) * kSub);
        }
    }
    for (uint32_t g = blockIdx.x * WPB + wave; g < n_groups; g += gstride) {
        const int64_t sbase = static_cast<int64_t>(g) * kSub;
        const int64_t ibase = a.in_off + sbase;
        const uint32_t c0 = C == 1 ? 0u : static_cast<uint32_t>((static_cast<uint64_t>(g) * (kSub % C) + lane2) % C);
        const uint32_t c1 = C == 1 ? 0u : (c0 + 1u) % C;
        const uint32_t cs[2] = {c0, c1};

        double F[2] = {1.0, 1.0}, sF[2] = {0.0, 0.0}, iF2[2] = {1.0, 1.0};
        if constexpr (FLAT) {
            if (a.flat_u8) {
                const uint32_t f = ld_u16(a.flat_u8 + sbase + lane2);
                const double2 f0 = t_flat[f & 255u], f1 = t_flat[f >> 8];
                F[0] = f0.x; iF2[0] = f0.y; F[1] = f1.x; iF2[1] = f1.y;
            } else {
                const f64x2 f = ld2(a.flat_f64 + sbase);
                F[0] = f.x; F[1] = f.y;
                if (STD) { iF2[0] = 1.0 / (F[0] * F[0]); iF2[1] = 1.0 / (F[1] * F[1]); }
            }
            if (STD) { const f64x2 f = ld2(a.flat_std + sbase); sF[0] = f.x; sF[1] = f.y; }
        }

        double S[2] = {0.0, 0.0}, acc[2] = {0.0, 0.0}, var[2] = {0.0, 0.0};
        if constexpr (!STD) {
            for (int i0 = 0; i0 < N; i0 += kF64Chunk) {
                f64x2 v[kF64Chunk];
#pragma unroll
                for (int k = 0; k < kF64Chunk; ++k)
                    if (i0 + k < N) v[k] = ld2(static_cast<const double*>(a.frame[i0 + k]) + ibase);
#pragma unroll
                for (int k = 0; k < kF64Chunk; ++k) {
                    if (i0 + k < N) {
                        const double it = a.inv_t[i0 + k];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const double x = j == 0 ? v[k].x : v[k].y;
                            const double dv = x - 0.5;
                            const double w = gauss_weight(dv);                            // measurand.py:615
                            const double gg = t_gd[lut_index(x) * C + cs[j]].x;
                            const double wg = w * gg;
                            if (i0 + k == 0) { S[j] = w; acc[j] = wg * it; }
                            else { S[j] += w; acc[j] = fma(wg, it, acc[j]); }                   // exposure_series.py:340, :388
                        }
                    }
                }
            }
            double val[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) val[j] = acc[j] / S[j];
            if constexpr (FLAT) {
                double dummy = 0.0;
                flat_field_math(F[0], iF2[0], 0.0, a.ff_mean[c0], 0.0, false, val[0], dummy);
                flat_field_math(F[1], iF2[1], 0.0, a.ff_mean[c1], 0.0, false, val[1], dummy);
            }
            if constexpr (SUMW) store2(a.out_sum_w + sbase, lane16, S[0], S[1]);
            store_pair<OUT>(out_at<OUT>(a.out_val, sbase), lane16, val[0], val[1]);
        } else {
            double invS[2], invS2[2];
            // one frame of pass 2 (measurand.py:512,616; exposure_series.py:388-389) given its weight
            auto pass2 = [&](int i, int j, double x, double w, double s, double it) {
                const double dw = gauss_dweight(x - 0.5, w);                                      // measurand.py:616
                const double2 gd = t_gd[lut_index(x) * C + cs[j]];
                const double gg = gd.x;
                const double wg = w * gg;
                const double dg = gd.y * s;                                                     // measurand.py:512
                const double term = merge_var_term(w, dw, gg, dg, invS[j], invS2[j], it);   // :389
                if (i == 0) { acc[j] = wg * it; var[j] = term * term; }
                else { acc[j] = fma(wg, it, acc[j]); var[j] = fma(term, term, var[j]); }
            };
            if (N <= kF64Keep) {
                // small stacks: the frame values stay in registers between the passes (re-reading them misses the
                // caches - 7 KB per wave-iteration, 20 waves per CU - and costs 56 B/element of extra traffic);
                // the weight is re-evaluated, exp() is not what bounds this kernel
                f64x2 v[kF64Keep];
                constexpr bool KEEPW = HM_F64_KEEP_W && !FLAT;   // (with the flat-field operands live as well the kept weights spill)
                double wk[KEEPW ? kF64Keep : 1][2];              // pass 1's weights, reused by pass 2 (one exp() per element-frame instead of two)
                if constexpr (PRE) {
                    // (unconditional: past the last group it re-reads the current one and the values are dropped - a branch around the loads
                    // would make the compiler wait for them before this group's arithmetic)
                    const int64_t nbase = a.in_off + static_cast<int64_t>(g + gstride < n_groups ? g + gstride : g) * kSub;
#pragma unroll
                    for (int i = 0; i < kF64Keep; ++i)
                        if (i < N) { v[i] = vpre[i]; vpre[i] = ld2(static_cast<const double*>(a.frame[i]) + nbase); }
                } else {
#pragma unroll
                    for (int i = 0; i < kF64Keep; ++i)
                        if (i < N) v[i] = ld2(static_cast<const double*>(a.frame[i]) + ibase);
                }
#pragma unroll
                for (int i = 0; i < kF64Keep; ++i) {
                    if (i < N) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const double w = gauss_weight((j == 0 ? v[i].x : v[i].y) - 0.5);
                            if constexpr (KEEPW) wk[i][j] = w;
                            if (i == 0) S[j] = w; else S[j] += w;
                        }
                        HM_PIN(S[0]); HM_PIN(S[1]);                 // one frame's exp() pair at a time: their temporaries,
                        __builtin_amdgcn_sched_barrier(0);          // interleaved across frames, are the register peak
                    }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) { invS[j] = 1.0 / S[j]; invS2[j] = 1.0 / (S[j] * S[j]); }
#pragma unroll
                for (int i = 0; i < kF64Keep; ++i) {
                    if (i < N) {
                        const f64x2 sdv = ld2(a.sd[i] + ibase);
                        const double it = a.inv_t[i];
                        if constexpr (KEEPW) {
                            pass2(i, 0, v[i].x, wk[i][0], sdv.x, it);
                            pass2(i, 1, v[i].y, wk[i][1], sdv.y, it);
                        } else {
                            pass2(i, 0, v[i].x, gauss_weight(v[i].x - 0.5), sdv.x, it);
                            pass2(i, 1, v[i].y, gauss_weight(v[i].y - 0.5), sdv.y, it);
                        }
                        HM_PIN(acc[0]); HM_PIN(acc[1]); HM_PIN(var[0]); HM_PIN(var[1]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            } else {
                for (int i0 = 0; i0 < N; i0 += kF64Chunk) {                                    // pass 1: S
                    f64x2 v[kF64Chunk];
#pragma unroll
                    for (int k = 0; k < kF64Chunk; ++k)
                        if (i0 + k < N) v[k] = ld2(static_cast<const double*>(a.frame[i0 + k]) + ibase);
#pragma unroll
                    for (int k = 0; k < kF64Chunk; ++k) {
                        if (i0 + k < N) {
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                const double dv = (j == 0 ? v[k].x : v[k].y) - 0.5;
                                const double w = gauss_weight(dv);
                                if (i0 + k == 0) S[j] = w; else S[j] += w;
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) { invS[j] = 1.0 / S[j]; invS2[j] = 1.0 / (S[j] * S[j]); }
                for (int i0 = 0; i0 < N; i0 += 2) {                                            // pass 2: weights re-evaluated
                    f64x2 v[2], sdv[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        if (i0 + k < N) {
                            v[k] = ld2(static_cast<const double*>(a.frame[i0 + k]) + ibase);
                            sdv[k] = ld2(a.sd[i0 + k] + ibase);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        if (i0 + k < N) {
                            const double it = a.inv_t[i0 + k];
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                const double x = j == 0 ? v[k].x : v[k].y;
                                const double dv = x - 0.5;
                                pass2(i0 + k, j, x, gauss_weight(dv), j == 0 ? sdv[k].x : sdv[k].y, it);
                            }
                        }
                    }
                }
            }
            double val[2], so[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) { val[j] = acc[j] / S[j]; so[j] = sqrt(var[j]); }
            if constexpr (FLAT) {
                flat_field_math(F[0], iF2[0], sF[0], a.ff_mean[c0], a.ff_std_mean[c0], true, val[0], so[0]);
                flat_field_math(F[1], iF2[1], sF[1], a.ff_mean[c1], a.ff_std_mean[c1], true, val[1], so[1]);
            }
            if constexpr (SUMW) store2(a.out_sum_w + sbase, lane16, S[0], S[1]);
            store_pair<OUT>(out_at<OUT>(a.out_val, sbase), lane16, val[0], val[1]);
            store_pair<OUT>(out_at<OUT>(a.out_std, sbase), lane16, so[0], so[1]);
        }
    }
}

// The two entry points differ in the occupancy the register allocator is asked for (A/B on one box, tools/ab3.sh):
// val-only runs best when it may use up to 168 VGPRs (3 waves/SIMD: more loads in flight per wave, 665 -> 599 us on
// 7 x 4096 x 4096 x 3); the std kernel ran best at 4 waves/SIMD while it re-evaluated its weights in pass 2 (127 VGPRs + 20 B
// scratch, 1 382 -> 1 343 us) and at 3 waves/SIMD now that it keeps them (HM_F64_KEEP_W; at 4 waves the kept weights spill: 1 566 us).
#ifndef HM_F64_VAL_WAVES
#define HM_F64_VAL_WAVES 3
#endif
#ifndef HM_F64_STD_WAVES
#define HM_F64_STD_WAVES 3
#endif
template <int C, bool FLAT, bool SUMW, int OUT = OUT_F64>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HM_F64_VAL_WAVES, HM_F64_VAL_WAVES))) void merge_f64_val(const MergeK a) {
    merge_f64_body<C, false, FLAT, SUMW, OUT>(a);
}
template <int C, bool FLAT, bool SUMW, int OUT = OUT_F64>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HM_F64_STD_WAVES, HM_F64_STD_WAVES))) void merge_f64_std(const MergeK a) {
    merge_f64_body<C, true, FLAT, SUMW, OUT>(a);
}

template <int C, int OUT>
static int launch_f64_c(const MergeK& k, bool with_std, hipStream_t st) {
    const bool flat = k.has_flat != 0, sumw = k.out_sum_w != nullptr;
    const int lds = 16 * 256 * C + (flat ? 16 * 256 : 0);
    const unsigned grid = stream_grid(k.n_elems / static_cast<int>(kSub), 4, 8);
    if (describe_only(with_std ? "merge_f64_std<C=%d,flat=%d,sum_w=%d>(N=%d)" : "merge_f64_val<C=%d,flat=%d,sum_w=%d>(N=%d)", C, flat, sumw, k.n_frames)) return HM_OK;
#define HM_F64(K, F, W) hipLaunchKernelGGL((K<C, F, W, OUT>), dim3(grid), dim3(256), lds, st, k)
    if (with_std) {
        if (flat && sumw) HM_F64(merge_f64_std, true, true); else if (flat) HM_F64(merge_f64_std, true, false);
        else if (sumw) HM_F64(merge_f64_std, false, true); else HM_F64(merge_f64_std, false, false);
    } else {
        if (flat && sumw) HM_F64(merge_f64_val, true, true); else if (flat) HM_F64(merge_f64_val, true, false);
        else if (sumw) HM_F64(merge_f64_val, false, true); else HM_F64(merge_f64_val, false, false);
    }
#undef HM_F64
    return launch_status();
}

template <int OUT>
int launch_f64(const MergeK& k, bool with_std, hipStream_t st) {
    switch (k.C) {
        case 1: return launch_f64_c<1, OUT>(k, with_std, st);
        case 2: return launch_f64_c<2, OUT>(k, with_std, st);
        case 3: return launch_f64_c<3, OUT>(k, with_std, st);
        default: return launch_f64_c<4, OUT>(k, with_std, st);
    }
}


// the instantiations the dispatcher links against (hm_merge_host.h declares them extern)
template int launch_f64<OUT_F64>(const MergeK&, bool, hipStream_t);
template int launch_f64<OUT_F32>(const MergeK&, bool, hipStream_t);

}  // namespace hm
