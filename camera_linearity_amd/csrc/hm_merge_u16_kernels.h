// hm_merge_u16_kernels.h - the kernel text and the launchers of the uint16 merge's two families (private to hm_merge_u16.hip, which
// instantiates them for value-only calls and float64 std frames, and hm_merge_u16_lut.hip, which instantiates the per-DN std table's
// forms: template flag LUT, MergeK::std_lut). The kernel map is at the head of hm_merge_u16.hip.
//
// LUT (hm_merge_u16_std_table; std calls only): frame i's std is std_lut[idx C + c] at the frame's own masked DN, so dg = icrf_diff * std is
// a per-(DN, channel) table entry and takes the place d has in the tables:
//   tab=lds           {w, dw}[n] | {g, d * std_lut}[n C]: the fill forms the product, pass 2 takes dg from the pair - no std stream, no multiply
//   tab=mixed-wdwdg   {w, dw}[n] | dg[n C] (the 8 (2 + C) n bytes of tab=mixed-wdwg), icrf gathered from global memory
//   tab=mixed-wdw, tab=global   icrf, icrf_diff and std_lut gathered from global memory, dg formed per element-frame from the same two operands
// The product is formed once from the same operands in every form (-ffp-contract=off): the bits of a std-frame call given the table's stds.
#pragma once
#include "hm_merge_u16.h"
#include "hm_merge_rules.h"
#include <mutex>

namespace hm {

constexpr int kU16Chunk = 8;          // frames whose loads a wave issues together (merge_u8_loop's kLoopChunk)
constexpr int kU16LdsBlock = 1024;    // threads of the tab=lds workgroup
constexpr int kU16GlobalBlock = 256;
constexpr int kU16LutPass2 = 4;       // LUT: frames per step of pass 2 (no std stream to keep in flight beside the frame words)

template <bool STD, int OUT, bool LUT = false>
__global__ __launch_bounds__(256) void merge_u16_generic(const MergeK a, const uint32_t mask) {
    static_assert(STD || !LUT, "the table stands for std frames");
    reset_hot_counters(a);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < a.n_elems; q += stride) {
        if constexpr (LUT) merge_u16_element<STD, OUT>(a, a.elem0 + q, U16FramesLut(a, mask, a.elem0 + q));
        else merge_u16_element<STD, OUT>(a, a.elem0 + q, U16Frames(a, mask, a.elem0 + q));
    }
}

// a.n_elems: whole groups of kSub elements, fewer than 2^32; the call keeps the pair rule (hdrmerge.h)
template <int PLACE, bool STD, int OUT, bool LUT = false>
__global__ __launch_bounds__(PLACE != hm_rules::U16_TAB_GLOBAL ? kU16LdsBlock : kU16GlobalBlock) void merge_u16_stream(const MergeK a, const uint32_t mask) {
    using namespace hm_rules;
    static_assert(STD || PLACE != U16_TAB_WDW_G, "value-only calls have the per-DN placement and the full one");
    static_assert(STD || !LUT, "the table stands for std frames");
    constexpr bool TABLDS = PLACE != U16_TAB_GLOBAL;          // the per-DN tables are in LDS
    constexpr bool ALL = PLACE == U16_TAB_ALL;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lane16 = lane * 16u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t n_groups = static_cast<uint32_t>(a.n_elems / kSub);
    const uint32_t gstride = gridDim.x * wpb;
    const int N = a.n_frames;
    const uint32_t C = static_cast<uint32_t>(a.C);
    const uint32_t n_dn = mask + 1u;                                      // rows of every table
    reset_hot_counters(a);

    if constexpr (TABLDS) {
        if constexpr (!STD) {
            double* t_w = reinterpret_cast<double*>(lds);
            for (uint32_t q = threadIdx.x; q < n_dn; q += blockDim.x) t_w[q] = a.w_lut[q];
            if constexpr (ALL) {
                double* t_wg = t_w + n_dn;
                for (uint32_t q = threadIdx.x; q < n_dn * C; q += blockDim.x) t_wg[q] = a.w_lut[q / C] * a.icrf[q];   // (w * g), exposure_series.py:388
            }
        } else {
            double2* t_wdw = reinterpret_cast<double2*>(lds);
            for (uint32_t q = threadIdx.x; q < n_dn; q += blockDim.x) t_wdw[q] = double2{a.w_lut[q], a.dw_lut[q]};
            if constexpr (ALL) {
                double2* t_gd = t_wdw + n_dn;
                for (uint32_t q = threadIdx.x; q < n_dn * C; q += blockDim.x) {
                    if constexpr (LUT) t_gd[q] = double2{a.icrf[q], a.icrf_diff[q] * a.std_lut[q]};                   // {g, dg}, measurand.py:512
                    else t_gd[q] = double2{a.icrf[q], a.icrf_diff[q]};
                }
            } else if constexpr (PLACE == U16_TAB_WDW_G) {
                double* t_g = reinterpret_cast<double*>(t_wdw + n_dn);
                for (uint32_t q = threadIdx.x; q < n_dn * C; q += blockDim.x) {
                    if constexpr (LUT) t_g[q] = a.icrf_diff[q] * a.std_lut[q];                                        // dg
                    else t_g[q] = a.icrf[q];
                }
            }
        }
        __syncthreads();
    }
    // the gathers, at masked indices only
    const auto get_w = [&](uint32_t idx) -> double {
        if constexpr (!TABLDS) return a.w_lut[idx];
        else if constexpr (!STD) return reinterpret_cast<const double*>(lds)[idx];
        else return reinterpret_cast<const double2*>(lds)[idx].x;
    };
    const auto get_val = [&](uint32_t idx, uint32_t c, double& w, double& wg) {
        if constexpr (ALL) {
            const double* t_w = reinterpret_cast<const double*>(lds);
            w = t_w[idx]; wg = t_w[n_dn + idx * C + c];
        } else {
            w = get_w(idx); wg = w * a.icrf[idx * C + c];
        }
    };
    // d: icrf_diff at the index - LUT: dg = icrf_diff * std_lut there
    const auto get_std = [&](uint32_t idx, uint32_t c, double& w, double& dw, double& g, double& d) {
        const double2* t_wdw = reinterpret_cast<const double2*>(lds);
        if constexpr (TABLDS) { const double2 x = t_wdw[idx]; w = x.x; dw = x.y; }
        else { w = a.w_lut[idx]; dw = a.dw_lut[idx]; }
        if constexpr (ALL) { const double2 y = t_wdw[n_dn + idx * C + c]; g = y.x; d = y.y; }
        else if constexpr (LUT) {
            g = a.icrf[idx * C + c];
            if constexpr (PLACE == U16_TAB_WDW_G) d = reinterpret_cast<const double*>(t_wdw + n_dn)[idx * C + c];
            else d = a.icrf_diff[idx * C + c] * a.std_lut[idx * C + c];                                               // measurand.py:512
        } else {
            if constexpr (PLACE == U16_TAB_WDW_G) g = reinterpret_cast<const double*>(t_wdw + n_dn)[idx * C + c];
            else g = a.icrf[idx * C + c];
            d = a.icrf_diff[idx * C + c];
        }
    };
    const auto ld_pair = [&](int i, int64_t ibase) -> uint32_t {          // the lane's two DNs of frame i: one 4-byte load
        return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(static_cast<const uint16_t*>(a.frame[i]) + ibase) + lane);
    };
    const auto ld_f64x2 = [&](const double* base) -> f64x2 {
        return __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(reinterpret_cast<const char*>(base) + lane16));
    };

    for (uint32_t g = blockIdx.x * wpb + wave; g < n_groups; g += gstride) {
        const int64_t sbase = static_cast<int64_t>(g) * kSub;             // relative to row0, scalar
        const int64_t ibase = a.in_off + sbase;
        const uint32_t c0 = (g * kSub + lane * 2u) % C;                   // element % C (fewer than 2^32 elements)
        const uint32_t c1 = c0 + 1u == C ? 0u : c0 + 1u;
        const uint32_t cs[2] = {c0, c1};

        double F[2] = {1.0, 1.0}, sF[2] = {0.0, 0.0}, iF2[2] = {1.0, 1.0};
        if (a.has_flat) {
            const f64x2 f = ld_f64x2(a.flat_f64 + sbase);
            F[0] = f.x; F[1] = f.y;
            if constexpr (STD) {
                iF2[0] = 1.0 / (F[0] * F[0]); iF2[1] = 1.0 / (F[1] * F[1]);
                const f64x2 s = ld_f64x2(a.flat_std + sbase);
                sF[0] = s.x; sF[1] = s.y;
            }
        }

        double S[2] = {0.0, 0.0}, acc[2] = {0.0, 0.0}, var[2] = {0.0, 0.0};
        if constexpr (!STD) {
            for (int i0 = 0; i0 < N; i0 += kU16Chunk) {
                uint32_t r[kU16Chunk];
#pragma unroll
                for (int k = 0; k < kU16Chunk; ++k)
                    if (i0 + k < N) r[k] = ld_pair(i0 + k, ibase);
#pragma unroll
                for (int k = 0; k < kU16Chunk; ++k) {
                    if (i0 + k < N) {
                        const double it = a.inv_t[i0 + k];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const uint32_t idx = (j == 0 ? r[k] : (r[k] >> 16)) & mask;
                            double w, wg;
                            get_val(idx, cs[j], w, wg);
                            if (i0 + k == 0) { S[j] = w; acc[j] = wg * it; }
                            else { S[j] += w; acc[j] = fma(wg, it, acc[j]); }            // exposure_series.py:340, :388
                        }
                    }
                }
            }
            double val[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) val[j] = acc[j] / S[j];
            if (a.has_flat) {
                double none = 0.0;
                flat_field_math(F[0], iF2[0], 0.0, a.ff_mean[c0], 0.0, false, val[0], none);
                flat_field_math(F[1], iF2[1], 0.0, a.ff_mean[c1], 0.0, false, val[1], none);
            }
            if (a.out_sum_w) store2(a.out_sum_w + sbase, lane16, S[0], S[1]);
            store_pair<OUT>(out_at<OUT>(a.out_val, sbase), lane16, val[0], val[1]);
        } else {
            // pass 1: S = sum_i w_i
            for (int i0 = 0; i0 < N; i0 += kU16Chunk) {
                uint32_t r[kU16Chunk];
#pragma unroll
                for (int k = 0; k < kU16Chunk; ++k)
                    if (i0 + k < N) r[k] = ld_pair(i0 + k, ibase);
#pragma unroll
                for (int k = 0; k < kU16Chunk; ++k) {
                    if (i0 + k < N) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const double w = get_w((j == 0 ? r[k] : (r[k] >> 16)) & mask);
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
            // pass 2: the frame words again (cache hits) + the float64 std streams, two frames per step (LUT: the frame words alone)
            constexpr int P2 = LUT ? kU16LutPass2 : 2;
            for (int i0 = 0; i0 < N; i0 += P2) {
                uint32_t r[P2];
                [[maybe_unused]] f64x2 sdv[P2];
#pragma unroll
                for (int k = 0; k < P2; ++k) {
                    if (i0 + k < N) {
                        r[k] = ld_pair(i0 + k, ibase);
                        if constexpr (!LUT) sdv[k] = ld_f64x2(a.sd[i0 + k] + ibase);
                    }
                }
#pragma unroll
                for (int k = 0; k < P2; ++k) {
                    if (i0 + k < N) {
                        const double it = a.inv_t[i0 + k];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const uint32_t idx = (j == 0 ? r[k] : (r[k] >> 16)) & mask;
                            double w, dw, gg, d;
                            get_std(idx, cs[j], w, dw, gg, d);
                            double dg;
                            if constexpr (LUT) dg = d;                                                     // the table's entry
                            else dg = d * (j == 0 ? sdv[k].x : sdv[k].y);                                  // measurand.py:512
                            // merge_var_term() of hm_merge_math.h, written out: called here, the std kernels schedule differently
                            const double A = (dw * gg + w * dg) * invS[j] - ((dw * w) * gg) * invS2[j];   // :389
                            const double term = (A * dg) * it;
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
            if (a.has_flat) {
                flat_field_math(F[0], iF2[0], sF[0], a.ff_mean[c0], a.ff_std_mean[c0], true, val[0], so[0]);
                flat_field_math(F[1], iF2[1], sF[1], a.ff_mean[c1], a.ff_std_mean[c1], true, val[1], so[1]);
            }
            if (a.out_sum_w) store2(a.out_sum_w + sbase, lane16, S[0], S[1]);
            store_pair<OUT>(out_at<OUT>(a.out_val, sbase), lane16, val[0], val[1]);
            store_pair<OUT>(out_at<OUT>(a.out_std, sbase), lane16, so[0], so[1]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// launchers (LUT: k.std_lut is set and the call forms a std)
// ------------------------------------------------------------------------------------------------
inline bool describe_u16(const char* kernel, const char* tab, int bits, const MergeK& k, bool with_std, bool lut) {
    if (!g_describe) return false;
    char fmt[160];
    const char* std_fmt = lut ? "lut" : with_std ? "1" : "0";
    if (tab) snprintf(fmt, sizeof fmt, "%s<tab=%s,bits=%d,C=%%d,std=%s,flat=%%d,sum_w=%%d>(N=%d)", kernel, tab, bits, std_fmt, k.n_frames);
    else snprintf(fmt, sizeof fmt, "%s<bits=%d,C=%%d,std=%s,flat=%%d,sum_w=%%d>(N=%d)", kernel, bits, std_fmt, k.n_frames);
    return describe_only(fmt, k.C, k.has_flat, k.out_sum_w != nullptr);
}

template <int OUT, bool LUT>
int launch_u16_generic(const MergeK& k, int bits, bool with_std, hipStream_t st) {
    if (LUT && !with_std) return HM_EINVAL;
    if (describe_u16("merge_u16_generic", nullptr, bits, k, with_std, LUT)) return HM_OK;
    const unsigned grid = stream_grid(k.n_elems, 256, 8);
    const uint32_t mask = (1u << bits) - 1u;
    if constexpr (LUT) hipLaunchKernelGGL((merge_u16_generic<true, OUT, true>), dim3(grid), dim3(256), 0, st, k, mask);
    else if (with_std) hipLaunchKernelGGL((merge_u16_generic<true, OUT>), dim3(grid), dim3(256), 0, st, k, mask);
    else hipLaunchKernelGGL((merge_u16_generic<false, OUT>), dim3(grid), dim3(256), 0, st, k, mask);
    return launch_status();
}

// More dynamic LDS than a kernel gets by default: every instantiation with tables in LDS is given the CU's 160 KiB, once per process, on
// the first launch of any of them (host-side, no stream work). One list per unit: the LUT forms are hm_merge_u16_lut.hip's.
#define HM_U16_FN(P, S, O) reinterpret_cast<const void*>(&merge_u16_stream<hm_rules::P, S, O, LUT>)
template <bool LUT>
int u16_lds_limit() {
    static std::once_flag once;
    static int status = HM_OK;
    std::call_once(once, [] {
        const void* fns[10];
        int n = 0;
        if constexpr (!LUT) {
            fns[n++] = HM_U16_FN(U16_TAB_ALL, false, OUT_F64); fns[n++] = HM_U16_FN(U16_TAB_ALL, false, OUT_F32);
            fns[n++] = HM_U16_FN(U16_TAB_PER_DN, false, OUT_F64); fns[n++] = HM_U16_FN(U16_TAB_PER_DN, false, OUT_F32);
        }
        fns[n++] = HM_U16_FN(U16_TAB_ALL, true, OUT_F64); fns[n++] = HM_U16_FN(U16_TAB_ALL, true, OUT_F32);
        fns[n++] = HM_U16_FN(U16_TAB_PER_DN, true, OUT_F64); fns[n++] = HM_U16_FN(U16_TAB_PER_DN, true, OUT_F32);
        fns[n++] = HM_U16_FN(U16_TAB_WDW_G, true, OUT_F64); fns[n++] = HM_U16_FN(U16_TAB_WDW_G, true, OUT_F32);
        for (int i = 0; i < n; ++i)
            if (hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds) != hipSuccess) { (void)hipGetLastError(); status = HM_ELAUNCH; }
    });
    return status;
}
#undef HM_U16_FN

// place: hm_rules::U16Tables
template <int OUT, bool LUT>
int launch_u16_stream(const MergeK& k, int bits, bool with_std, int place, hipStream_t st) {
    using namespace hm_rules;
    if (LUT && !with_std) return HM_EINVAL;
    const char* tab = place == U16_TAB_ALL ? "lds" : place == U16_TAB_WDW_G ? (LUT ? "mixed-wdwdg" : "mixed-wdwg")
                      : place == U16_TAB_PER_DN ? (with_std ? "mixed-wdw" : "mixed-w") : "global";
    if (describe_u16("merge_u16_stream", tab, bits, k, with_std, LUT)) return HM_OK;
    const uint32_t mask = (1u << bits) - 1u;
    const int64_t groups = k.n_elems / static_cast<int>(kSub);
    if (place != U16_TAB_GLOBAL) {
        const int rc = u16_lds_limit<LUT>();
        if (rc != HM_OK) return rc;
        const unsigned lds = static_cast<unsigned>(u16_table_bytes(bits, k.C, with_std, place));
        const unsigned grid = stream_grid(groups, kU16LdsBlock / kWave, 1);     // one workgroup per CU at the most, none without a group
#define HM_U16_LAUNCH(P, S) hipLaunchKernelGGL((merge_u16_stream<P, S, OUT, LUT>), dim3(grid), dim3(kU16LdsBlock), lds, st, k, mask)
        if constexpr (LUT) {
            if (place == U16_TAB_ALL) HM_U16_LAUNCH(U16_TAB_ALL, true);
            else if (place == U16_TAB_WDW_G) HM_U16_LAUNCH(U16_TAB_WDW_G, true);
            else HM_U16_LAUNCH(U16_TAB_PER_DN, true);
        } else {
            if (place == U16_TAB_ALL) { if (with_std) HM_U16_LAUNCH(U16_TAB_ALL, true); else HM_U16_LAUNCH(U16_TAB_ALL, false); }
            else if (place == U16_TAB_WDW_G) { if (!with_std) return HM_EINVAL; HM_U16_LAUNCH(U16_TAB_WDW_G, true); }
            else { if (with_std) HM_U16_LAUNCH(U16_TAB_PER_DN, true); else HM_U16_LAUNCH(U16_TAB_PER_DN, false); }
        }
#undef HM_U16_LAUNCH
    } else {
        const unsigned grid = stream_grid(groups, kU16GlobalBlock / kWave, 8);
        if constexpr (LUT) hipLaunchKernelGGL((merge_u16_stream<U16_TAB_GLOBAL, true, OUT, true>), dim3(grid), dim3(kU16GlobalBlock), 0, st, k, mask);
        else if (with_std) hipLaunchKernelGGL((merge_u16_stream<U16_TAB_GLOBAL, true, OUT>), dim3(grid), dim3(kU16GlobalBlock), 0, st, k, mask);
        else hipLaunchKernelGGL((merge_u16_stream<U16_TAB_GLOBAL, false, OUT>), dim3(grid), dim3(kU16GlobalBlock), 0, st, k, mask);
    }
    return launch_status();
}

// the table forms are hm_merge_u16_lut.hip's: no other unit instantiates them, or the kernels behind them
#define HM_EXTERN_U16_LUT(OUT) \
    extern template int launch_u16_generic<OUT, true>(const MergeK&, int, bool, hipStream_t); \
    extern template int launch_u16_stream<OUT, true>(const MergeK&, int, bool, int, hipStream_t);
HM_EXTERN_U16_LUT(OUT_F64)
HM_EXTERN_U16_LUT(OUT_F32)
#undef HM_EXTERN_U16_LUT

}  // namespace hm
