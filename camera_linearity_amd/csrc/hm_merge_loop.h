// hm_merge_loop.h - merge_u8_loop / merge_u8_loop_std: the fused merge's streaming kernels for uint8 frames with the frame count and the
// channel count as run-time values (gfx950), with launch_loop. The kernel map of the whole merge is in hm_merge.hip. Nothing here is
// instantiated by including it: hm_merge_loop.hip instantiates launch_loop for float64 std frames (and the val-only and table kernels),
// hm_merge_loop_sd32.hip for float32 std frames (hm_merge_std_f32).
#pragma once
#include "hm_merge_host.h"

namespace hm {

// ------------------------------------------------------------------------------------------------
// merge_u8_loop: the same work decomposition and arithmetic as merge_u8_fast with the frame count as a run-time
// value, for 16 < N <= HM_MAX_FRAMES (the templated kernel is instantiated for N <= 16; before this kernel larger
// stacks fell to merge_generic at 0.19-0.33 of the HBM roofline, tools/bench_n.py). Frames are consumed in chunks
// of kLoopChunk: the chunk's ushort loads are issued together (frame pointers and 1/t come from the kernarg segment
// through scalar loads with a uniform index), then its LDS gathers, then the accumulation in frame order. The std
// variant re-reads the frame bytes in its second pass (L2 hits, 1 byte per element-frame) instead of keeping N
// packed words in registers. No cross-group prefetch: the kernel stays under 64 VGPRs and relies on 8 waves/SIMD.
// ------------------------------------------------------------------------------------------------
constexpr int kLoopChunk = 8;


// SD (hm_merge_std_f32): element type of the std frames (float: 8-byte pair loads, widened once in registers)
template <int C, bool STD, bool FLAT, bool SUMW, int OUT, bool LUT = false, typename SD = double>
__device__ __forceinline__ void merge_u8_loop_body(const MergeK& a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    reset_hot_counters(a);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lane2 = lane * 2u, lane16 = lane * 16u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr uint32_t WPB = 4;
    const uint32_t n_groups = static_cast<uint32_t>(a.n_elems / kSub);
    const uint32_t gstride = gridDim.x * WPB;
    const int N = a.n_frames;

    if constexpr (!STD) {
        for (int q = threadIdx.x; q < 256 * C; q += 256) {
            const double w = a.w_lut[q / C];
            reinterpret_cast<double2*>(lds)[q] = double2{w, w * a.icrf[q]};      // {w, w * g}, exposure_series.py:388
        }
    } else {
        double2* t_wdw = reinterpret_cast<double2*>(lds);
        double2* t_gd = reinterpret_cast<double2*>(lds + 16 * 256);
        for (int i = threadIdx.x; i < 256; i += 256) t_wdw[i] = double2{a.w_lut[i], a.dw_lut[i]};
        // LUT (hm_merge_std_table): {g, dg = icrf_diff * std} per (DN, c), as in merge_u8_fast_body
        for (int i = threadIdx.x; i < 256 * C; i += 256) t_gd[i] = double2{a.icrf[i], LUT ? a.icrf_diff[i] * a.std_lut[i] : a.icrf_diff[i]};
    }
    double2* t_flat = reinterpret_cast<double2*>(lds + (STD ? 16 * 256 + 16 * 256 * C : 16 * 256 * C));
    if constexpr (FLAT) {
        for (int i = threadIdx.x; i < 256; i += 256) {
            const double F = static_cast<double>(i) / 255.0;
            t_flat[i] = double2{F, 1.0 / (F * F)};
        }
    }
    __syncthreads();

    for (uint32_t g = blockIdx.x * WPB + wave; g < n_groups; g += gstride) {
        const int64_t sbase = static_cast<int64_t>(g) * kSub;                 // relative to row0, scalar
        const int64_t ibase = a.in_off + sbase;
        const uint32_t c0 = C == 1 ? 0u : static_cast<uint32_t>((static_cast<uint64_t>(g) * (kSub % C) + lane2) % C);   // element % C
        const uint32_t c1 = C == 1 ? 0u : (c0 + 1u) % C;
        const uint32_t coffs[2] = {c0 * 16u, c1 * 16u};

        double F[2] = {1.0, 1.0}, sF[2] = {0.0, 0.0}, iF2[2] = {1.0, 1.0};
        if constexpr (FLAT) {
            if (a.flat_u8) {
                const uint32_t f = ld_u16(a.flat_u8 + sbase + lane2);
                const double2 f0 = t_flat[f & 255u], f1 = t_flat[f >> 8];
                F[0] = f0.x; iF2[0] = f0.y; F[1] = f1.x; iF2[1] = f1.y;
            } else {
                const f64x2 f = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(reinterpret_cast<const char*>(a.flat_f64 + sbase) + lane16));
                F[0] = f.x; F[1] = f.y;
                if (STD) { iF2[0] = 1.0 / (F[0] * F[0]); iF2[1] = 1.0 / (F[1] * F[1]); }
            }
            if (STD) {
                const f64x2 f = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(reinterpret_cast<const char*>(a.flat_std + sbase) + lane16));
                sF[0] = f.x; sF[1] = f.y;
            }
        }

        double S[2] = {0.0, 0.0}, acc[2] = {0.0, 0.0}, var[2] = {0.0, 0.0};
        if constexpr (!STD) {
            for (int i0 = 0; i0 < N; i0 += kLoopChunk) {
                uint32_t r[kLoopChunk];
#pragma unroll
                for (int k = 0; k < kLoopChunk; ++k)
                    if (i0 + k < N) r[k] = ld_u16(static_cast<const uint8_t*>(a.frame[i0 + k]) + ibase + lane2);
#pragma unroll
                for (int k = 0; k < kLoopChunk; ++k) {
                    if (i0 + k < N) {
                        const double it = a.inv_t[i0 + k];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const uint32_t dn = j == 0 ? (r[k] & 255u) : (r[k] >> 8);
                            const double2 tw = *reinterpret_cast<const double2*>(lds + dn * (16u * C) + coffs[j]);
                            const double w = tw.x, wg = tw.y;
                            if (i0 + k == 0) { S[j] = w; acc[j] = wg * it; }
                            else { S[j] += w; acc[j] = fma(wg, it, acc[j]); }            // exposure_series.py:340, :388
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
            const double2* t_wdw = reinterpret_cast<const double2*>(lds);
            const char* t_gd = lds + 16 * 256;
            // pass 1: S = sum_i w_i
            for (int i0 = 0; i0 < N; i0 += kLoopChunk) {
                uint32_t r[kLoopChunk];
#pragma unroll
                for (int k = 0; k < kLoopChunk; ++k)
                    if (i0 + k < N) r[k] = ld_u16(static_cast<const uint8_t*>(a.frame[i0 + k]) + ibase + lane2);
#pragma unroll
                for (int k = 0; k < kLoopChunk; ++k) {
                    if (i0 + k < N) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const double w = t_wdw[j == 0 ? (r[k] & 255u) : (r[k] >> 8)].x;
                            if (i0 + k == 0) S[j] = w; else S[j] += w;
                        }
                    }
                }
            }
            double invS[2], invS2[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                invS[j] = 1.0 / S[j];
                invS2[j] = 1.0 / (S[j] * S[j]);                          // 1 / S**2, exposure_series.py:343
            }
            // pass 2: the frame bytes again (cache hits) + the float64 std streams, two frames per step (LUT: no std streams, P2 = 4 frames)
            constexpr int P2 = LUT ? 4 : 2;
            for (int i0 = 0; i0 < N; i0 += P2) {
                uint32_t r[P2];
                typename SdPair<SD>::type sdv[P2];
#pragma unroll
                for (int k = 0; k < P2; ++k) {
                    if (i0 + k < N) {
                        r[k] = ld_u16(static_cast<const uint8_t*>(a.frame[i0 + k]) + ibase + lane2);
                        if constexpr (LUT) sdv[k] = typename SdPair<SD>::type{1.0, 1.0};      // unused: the table entry is dg
                        else sdv[k] = ld_sd_pair<SD>(a.template sd_as<SD>(i0 + k) + ibase, lane16);
                    }
                }
#pragma unroll
                for (int k = 0; k < P2; ++k) {
                    if (i0 + k < N) {
                        const double it = a.inv_t[i0 + k];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const uint32_t dn = j == 0 ? (r[k] & 255u) : (r[k] >> 8);
                            const double2 wdw = t_wdw[dn];
                            const double2 gd = *reinterpret_cast<const double2*>(t_gd + dn * (16u * C) + coffs[j]);
                            const double w = wdw.x, dw = wdw.y, gg = gd.x;
                            const double dg = LUT ? gd.y : gd.y * static_cast<double>(j == 0 ? sdv[k].x : sdv[k].y);   // measurand.py:512
                            const double term = merge_var_term(w, dw, gg, dg, invS[j], invS2[j], it);   // :389
                            if (i0 + k == 0) { acc[j] = (w * gg) * it; var[j] = term * term; }
                            else {
                                acc[j] = fma(w * gg, it, acc[j]);                                          // :388
                                var[j] = fma(term, term, var[j]);
                            }
                        }
                    }
                }
            }
            double val[2], so[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                val[j] = acc[j] / S[j];
                so[j] = sqrt(var[j]);                                                                      // :394
            }
            if constexpr (FLAT) {
                flat_field_math(F[0], iF2[0], sF[0], a.ff_mean[c0], a.ff_std_mean[c0], true, val[0], so[0]);
                flat_field_math(F[1], iF2[1], sF[1], a.ff_mean[c1], a.ff_std_mean[c1], true, val[1], so[1]);
            }
            // (the table and float32-std instantiations exist with SUMW only and test the pointer - a scalar branch - instead of doubling their number: build time)
            if constexpr (SUMW) { if ((!LUT && std::is_same_v<SD, double>) || a.out_sum_w) store2(a.out_sum_w + sbase, lane16, S[0], S[1]); }
            store_pair<OUT>(out_at<OUT>(a.out_val, sbase), lane16, val[0], val[1]);
            store_pair<OUT>(out_at<OUT>(a.out_std, sbase), lane16, so[0], so[1]);
        }
    }
}

#ifdef HM_LOOP_VAL_WAVES
#define HM_LOOP_VAL_ATTR __attribute__((amdgpu_waves_per_eu(HM_LOOP_VAL_WAVES, HM_LOOP_VAL_WAVES)))
#else
#define HM_LOOP_VAL_ATTR
#endif
#ifdef HM_LOOP_STD_WAVES
#define HM_LOOP_STD_ATTR __attribute__((amdgpu_waves_per_eu(HM_LOOP_STD_WAVES, HM_LOOP_STD_WAVES)))
#else
#define HM_LOOP_STD_ATTR
#endif
template <int C, bool FLAT, bool SUMW, int OUT = OUT_F64>
__global__ __launch_bounds__(256) HM_LOOP_VAL_ATTR void merge_u8_loop(const MergeK a) { merge_u8_loop_body<C, false, FLAT, SUMW, OUT>(a); }
template <int C, bool FLAT, bool SUMW, int OUT = OUT_F64, bool LUT = false, typename SD = double>
__global__ __launch_bounds__(256) HM_LOOP_STD_ATTR void merge_u8_loop_std(const MergeK a) { merge_u8_loop_body<C, true, FLAT, SUMW, OUT, LUT, SD>(a); }

template <int C, int OUT, typename SD>
static int launch_loop_c(const MergeK& k, bool with_std, hipStream_t st) {
    const bool flat = k.has_flat != 0, sumw = k.out_sum_w != nullptr;
    const int lds = (with_std ? 16 * 256 + 16 * 256 * C : 16 * 256 * C) + (flat ? 16 * 256 : 0);
    const unsigned grid = stream_grid(k.n_elems / static_cast<int>(kSub), 4, 8);
    if (describe_only(with_std ? "merge_u8_loop_std<C=%d,flat=%d,sum_w=%d>(N=%d)" : "merge_u8_loop<C=%d,flat=%d,sum_w=%d>(N=%d)", C, flat, sumw, k.n_frames)) return HM_OK;
#define HM_LOOP(K, F, W) hipLaunchKernelGGL((K<C, F, W, OUT>), dim3(grid), dim3(256), lds, st, k)
#define HM_LOOP_LUT(F) hipLaunchKernelGGL((merge_u8_loop_std<C, F, true, OUT, true>), dim3(grid), dim3(256), lds, st, k)
    if constexpr (std::is_same_v<SD, float>) {    // hm_merge_std_f32 (the dispatcher sends std calls only; one instantiation serves calls with and without out_sum_w)
        if (!with_std || k.std_lut) return HM_EINVAL;
        if (flat) hipLaunchKernelGGL((merge_u8_loop_std<C, true, true, OUT, false, float>), dim3(grid), dim3(256), lds, st, k);
        else hipLaunchKernelGGL((merge_u8_loop_std<C, false, true, OUT, false, float>), dim3(grid), dim3(256), lds, st, k);
    } else if (with_std && k.std_lut) {                  // (one instantiation serves calls with and without out_sum_w)
        if (flat) HM_LOOP_LUT(true); else HM_LOOP_LUT(false);
    } else if (with_std) {
        if (flat && sumw) HM_LOOP(merge_u8_loop_std, true, true); else if (flat) HM_LOOP(merge_u8_loop_std, true, false);
        else if (sumw) HM_LOOP(merge_u8_loop_std, false, true); else HM_LOOP(merge_u8_loop_std, false, false);
    } else {
        if (flat && sumw) HM_LOOP(merge_u8_loop, true, true); else if (flat) HM_LOOP(merge_u8_loop, true, false);
        else if (sumw) HM_LOOP(merge_u8_loop, false, true); else HM_LOOP(merge_u8_loop, false, false);
    }
#undef HM_LOOP_LUT
#undef HM_LOOP
    return launch_status();
}

template <int OUT, typename SD>
int launch_loop(const MergeK& k, bool with_std, hipStream_t st) {
    switch (k.C) {
        case 1: return launch_loop_c<1, OUT, SD>(k, with_std, st);
        case 2: return launch_loop_c<2, OUT, SD>(k, with_std, st);
        case 3: return launch_loop_c<3, OUT, SD>(k, with_std, st);
        default: return launch_loop_c<4, OUT, SD>(k, with_std, st);
    }
}

}  // namespace hm
