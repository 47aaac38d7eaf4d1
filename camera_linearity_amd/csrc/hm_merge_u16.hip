// hm_merge_u16.hip - the fused merge for 9- to 16-bit cameras (gfx950): uint16 DN frames, an explicit bit depth, per-DN tables of
// 2^bit_depth rows (hdrmerge.h: hm_merge_u16). The kernel map of the 8-bit merge is in hm_merge.hip; this unit holds its own family, the
// dispatch and the C entry points. The argument rules are hm_merge_rules.h's ENTRY_U16 (shared with the host build).
//
//   merge_u16_generic   one element per thread, tables gathered from global memory: any alignment, the tails, variant = -1, the
//                       sum-of-weights-only call. merge_generic with 2-byte loads and table pointers that address global memory.
//   merge_u16_stream    merge_u8_loop / merge_u8_loop_std's decomposition at run-time N and C: a wave owns groups of 128 consecutive
//                       elements, a lane two of them - one 4-byte load per frame, 16-byte stores - frames in chunks of kU16Chunk.
//                       Template parameter PLACE (hm_rules::U16Tables) says where the tables live:
//                         tab=lds     dynamic LDS, value-only w[2^b] | (w g)[2^b C] (8 (1 + C) 2^b bytes), with std {w, dw}[2^b] |
//                                     {g, d}[2^b C] (16 (1 + C) 2^b bytes); chosen when that is at most 160 KiB (hm_rules::u16_tables_fit_lds).
//                                     One workgroup of 1024 threads owns the CU (16 waves cover the gather latency; __launch_bounds__(1024)
//                                     keeps the kernel at 128 registers); the grid is no larger than the number of 16-group blocks of the
//                                     call, so a small image does not fill a table per CU for nothing.
//                         tab=mixed-wdwg / mixed-wdw / mixed-w   the largest part that fits where not everything does: {w, dw} and g
//                                     (std calls; icrf_diff gathered from global memory), or the per-DN tables alone ({w, dw} / w; the
//                                     per-(DN, channel) tables from global memory). Same workgroup shape as tab=lds.
//                         tab=global  the same loop with every gather going through L1 / L2: what is left (16 bits always).
// Every table access - LDS or global - is at idx = DN & (2^bit_depth - 1): stray high bits never read outside a table.
// One operation sequence per output element in every kernel, merge_one_element's (hm_merge_dev.h): S in frame order, 1/S and 1/S**2 once,
// the numerator and the variance terms accumulated with fma in frame order, the product w g formed once (a table entry or a register).
// hm_merge_u16_darks adds the hot-pixel pass of hm_merge_u16_hot.hip after these kernels (ENTRY_U16_DARKS): they never read a dark map; the
// first of them zeroes the hot-pixel queue's counters in passing (MergeK::hot_reset, NULL in every hm_merge_u16 call).
#include "hm_merge_u16.h"
#include "hm_merge_rules.h"
#include <mutex>

namespace hm {

constexpr int kU16Chunk = 8;          // frames whose loads a wave issues together (merge_u8_loop's kLoopChunk)
constexpr int kU16LdsBlock = 1024;    // threads of the tab=lds workgroup
constexpr int kU16GlobalBlock = 256;

template <bool STD, int OUT>
__global__ __launch_bounds__(256) void merge_u16_generic(const MergeK a, const uint32_t mask) {
    reset_hot_counters(a);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < a.n_elems; q += stride)
        merge_u16_element<STD, OUT>(a, a.elem0 + q, U16Frames(a, mask, a.elem0 + q));
}

// a.n_elems: whole groups of kSub elements, fewer than 2^32; the call keeps the pair rule (hdrmerge.h)
template <int PLACE, bool STD, int OUT>
__global__ __launch_bounds__(PLACE != hm_rules::U16_TAB_GLOBAL ? kU16LdsBlock : kU16GlobalBlock) void merge_u16_stream(const MergeK a, const uint32_t mask) {
    using namespace hm_rules;
    static_assert(STD || PLACE != U16_TAB_WDW_G, "value-only calls have the per-DN placement and the full one");
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
                for (uint32_t q = threadIdx.x; q < n_dn * C; q += blockDim.x) t_gd[q] = double2{a.icrf[q], a.icrf_diff[q]};
            } else if constexpr (PLACE == U16_TAB_WDW_G) {
                double* t_g = reinterpret_cast<double*>(t_wdw + n_dn);
                for (uint32_t q = threadIdx.x; q < n_dn * C; q += blockDim.x) t_g[q] = a.icrf[q];
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
    const auto get_std = [&](uint32_t idx, uint32_t c, double& w, double& dw, double& g, double& d) {
        const double2* t_wdw = reinterpret_cast<const double2*>(lds);
        if constexpr (TABLDS) { const double2 x = t_wdw[idx]; w = x.x; dw = x.y; }
        else { w = a.w_lut[idx]; dw = a.dw_lut[idx]; }
        if constexpr (ALL) { const double2 y = t_wdw[n_dn + idx * C + c]; g = y.x; d = y.y; }
        else {
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
            // pass 2: the frame words again (cache hits) + the float64 std streams, two frames per step
            constexpr int P2 = 2;
            for (int i0 = 0; i0 < N; i0 += P2) {
                uint32_t r[P2];
                f64x2 sdv[P2];
#pragma unroll
                for (int k = 0; k < P2; ++k) {
                    if (i0 + k < N) {
                        r[k] = ld_pair(i0 + k, ibase);
                        sdv[k] = ld_f64x2(a.sd[i0 + k] + ibase);
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
                            const double dg = d * (j == 0 ? sdv[k].x : sdv[k].y);                          // measurand.py:512
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
// launchers
// ------------------------------------------------------------------------------------------------
static bool describe_u16(const char* kernel, const char* tab, int bits, const MergeK& k, bool with_std) {
    if (!g_describe) return false;
    char fmt[160];
    if (tab) snprintf(fmt, sizeof fmt, "%s<tab=%s,bits=%d,C=%%d,std=%%d,flat=%%d,sum_w=%%d>(N=%d)", kernel, tab, bits, k.n_frames);
    else snprintf(fmt, sizeof fmt, "%s<bits=%d,C=%%d,std=%%d,flat=%%d,sum_w=%%d>(N=%d)", kernel, bits, k.n_frames);
    return describe_only(fmt, k.C, with_std, k.has_flat, k.out_sum_w != nullptr);
}

template <int OUT>
static int launch_u16_generic(const MergeK& k, int bits, bool with_std, hipStream_t st) {
    if (describe_u16("merge_u16_generic", nullptr, bits, k, with_std)) return HM_OK;
    const unsigned grid = stream_grid(k.n_elems, 256, 8);
    const uint32_t mask = (1u << bits) - 1u;
    if (with_std) hipLaunchKernelGGL((merge_u16_generic<true, OUT>), dim3(grid), dim3(256), 0, st, k, mask);
    else hipLaunchKernelGGL((merge_u16_generic<false, OUT>), dim3(grid), dim3(256), 0, st, k, mask);
    return launch_status();
}

// More dynamic LDS than a kernel gets by default: every tab=lds instantiation is given the CU's 160 KiB, once per process, on the first
// launch of any of them (host-side, no stream work).
#define HM_U16_FN(P, S, O) reinterpret_cast<const void*>(&merge_u16_stream<hm_rules::P, S, O>)
static int u16_lds_limit() {
    static std::once_flag once;
    static int status = HM_OK;
    std::call_once(once, [] {
        const void* fns[] = {HM_U16_FN(U16_TAB_ALL, false, OUT_F64), HM_U16_FN(U16_TAB_ALL, true, OUT_F64), HM_U16_FN(U16_TAB_ALL, false, OUT_F32),
                             HM_U16_FN(U16_TAB_ALL, true, OUT_F32), HM_U16_FN(U16_TAB_PER_DN, false, OUT_F64), HM_U16_FN(U16_TAB_PER_DN, true, OUT_F64),
                             HM_U16_FN(U16_TAB_PER_DN, false, OUT_F32), HM_U16_FN(U16_TAB_PER_DN, true, OUT_F32), HM_U16_FN(U16_TAB_WDW_G, true, OUT_F64),
                             HM_U16_FN(U16_TAB_WDW_G, true, OUT_F32)};
        for (const void* fn : fns)
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds) != hipSuccess) { (void)hipGetLastError(); status = HM_ELAUNCH; }
    });
    return status;
}
#undef HM_U16_FN

// place: hm_rules::U16Tables
template <int OUT>
static int launch_u16_stream(const MergeK& k, int bits, bool with_std, int place, hipStream_t st) {
    using namespace hm_rules;
    const char* tab = place == U16_TAB_ALL ? "lds" : place == U16_TAB_WDW_G ? "mixed-wdwg" : place == U16_TAB_PER_DN ? (with_std ? "mixed-wdw" : "mixed-w") : "global";
    if (describe_u16("merge_u16_stream", tab, bits, k, with_std)) return HM_OK;
    const uint32_t mask = (1u << bits) - 1u;
    const int64_t groups = k.n_elems / static_cast<int>(kSub);
    if (place != U16_TAB_GLOBAL) {
        const int rc = u16_lds_limit();
        if (rc != HM_OK) return rc;
        const unsigned lds = static_cast<unsigned>(u16_table_bytes(bits, k.C, with_std, place));
        const unsigned grid = stream_grid(groups, kU16LdsBlock / kWave, 1);     // one workgroup per CU at the most, none without a group
#define HM_U16_LAUNCH(P, S) hipLaunchKernelGGL((merge_u16_stream<P, S, OUT>), dim3(grid), dim3(kU16LdsBlock), lds, st, k, mask)
        if (place == U16_TAB_ALL) { if (with_std) HM_U16_LAUNCH(U16_TAB_ALL, true); else HM_U16_LAUNCH(U16_TAB_ALL, false); }
        else if (place == U16_TAB_WDW_G) { if (!with_std) return HM_EINVAL; HM_U16_LAUNCH(U16_TAB_WDW_G, true); }
        else { if (with_std) HM_U16_LAUNCH(U16_TAB_PER_DN, true); else HM_U16_LAUNCH(U16_TAB_PER_DN, false); }
#undef HM_U16_LAUNCH
    } else {
        const unsigned grid = stream_grid(groups, kU16GlobalBlock / kWave, 8);
        if (with_std) hipLaunchKernelGGL((merge_u16_stream<U16_TAB_GLOBAL, true, OUT>), dim3(grid), dim3(kU16GlobalBlock), 0, st, k, mask);
        else hipLaunchKernelGGL((merge_u16_stream<U16_TAB_GLOBAL, false, OUT>), dim3(grid), dim3(kU16GlobalBlock), 0, st, k, mask);
    }
    return launch_status();
}

// The library's choice of the table placement (variant = 0): everything in LDS where it fits, else the largest part that does
// (measured: DESIGN.md 4.1.5).
static int u16_default_tables(int bits, int C, bool with_std) {
    return hm_rules::u16_tables_fit_lds(bits, C, with_std) ? hm_rules::U16_TAB_ALL : hm_rules::u16_mixed_tables(bits, C, with_std);
}

template <int OUT>
static int merge_u16_launch(const hm_rules::MergeCall& call, void* stream) {
    const hm_merge_args* g = &call.a;
    const int N = g->n_frames, C = g->channels, bits = call.bit_depth;
    const bool with_std = call.with_std && g->out_val, flat = call.flat, hot = call.hot;
    MergeK k{};
    for (int i = 0; i < N; ++i) {
        k.frame[i] = call.frames_u16[i];
        if (g->stds) k.sd[i] = g->stds[i];
        k.inv_t[i] = 1.0 / g->exposures[i];
        k.dark[i] = hot ? reinterpret_cast<const uint8_t*>(call.darks_u16[i]) : nullptr;       // read through dark_as<uint16_t>()
        k.dark_min[i] = hot && call.darks_u16[i] ? g->dark_min_dn[i] : 1 << 16;
    }
    k.icrf = g->icrf; k.icrf_diff = g->icrf_diff; k.w_lut = g->w_lut; k.dw_lut = g->dw_lut;
    k.flat_f64 = g->flat_f64; k.flat_std = g->flat_std;
    for (int c = 0; c < HM_MAX_CHANNELS; ++c) { k.ff_mean[c] = g->ff_mean[c]; k.ff_std_mean[c] = g->ff_std_mean[c]; }
    k.out_val = g->out_val; k.out_std = g->out_std; k.out_sum_w = g->out_sum_w;
    const int64_t E = g->rows * g->width * C;
    k.n_elems = E; k.elem0 = 0;
    k.in_off = (g->row0 - g->buf_row0) * g->width * C;
    k.H = g->height; k.W = g->width; k.row0 = g->row0; k.buf_row0 = g->buf_row0; k.buf_rows = g->buf_rows;
    k.n_frames = N; k.C = C; k.median_k = hot ? g->median_k : 3; k.has_flat = flat ? 1 : 0;
    k.variant = g->variant; k.inv_t_inrange = 1;
    hipStream_t st = as_stream(stream);
    // the hot-pixel pass's queue: the caller's workspace where it is usable (hm_merge's rule), else the pass tests every element itself
    const bool hot_queue = hot && g->hot_workspace && g->hot_workspace_bytes >= hm_merge_hot_workspace_min_bytes(E) &&
                           aligned(g->hot_workspace, 16) && E < (int64_t{1} << 32);
    k.hot_reset = hot_queue ? static_cast<uint32_t*>(g->hot_workspace) : nullptr;
    const auto hot_pass = [&]() {
        if (!hot) return static_cast<int>(HM_OK);
        return launch_u16_hot(k, bits, with_std, OUT == OUT_F32, hot_queue ? static_cast<uint32_t*>(g->hot_workspace) : nullptr,
                              hot_queue ? g->hot_workspace_bytes : 0, st);
    };

    // the pair rule (hdrmerge.h): 4-byte frame words, 16-byte float64 pairs (8-byte float32 ones)
    bool fast = g->out_val && E < (int64_t{1} << 32) && g->variant >= 0;
    for (int i = 0; i < N && fast; ++i) {
        fast = aligned(call.frames_u16[i] + k.in_off, 4);
        if (fast && with_std) fast = aligned(k.sd[i] + k.in_off, 16);
    }
    constexpr int pair_bytes = OUT == OUT_F32 ? 8 : 16;
    fast = fast && aligned(k.out_val, pair_bytes) && (!k.out_std || aligned(k.out_std, pair_bytes)) && (!k.out_sum_w || aligned(k.out_sum_w, 16));
    if (fast && flat) fast = aligned(k.flat_f64, 16) && (!with_std || aligned(k.flat_std, 16));
    if (!fast) {
        const int rc = launch_u16_generic<OUT>(k, bits, with_std, st);
        return rc != HM_OK ? rc : hot_pass();
    }

    // (variants 1 and 3 that do not fit: refused by the rules)
    const int place = g->variant == 1 ? hm_rules::U16_TAB_ALL : g->variant == 2 ? hm_rules::U16_TAB_GLOBAL
                      : g->variant == 3 ? hm_rules::u16_mixed_tables(bits, C, with_std) : u16_default_tables(bits, C, with_std);
    const int64_t body = (E / kSub) * kSub;
    if (body > 0) {
        MergeK kb = k;
        kb.n_elems = body;
        const int rc = launch_u16_stream<OUT>(kb, bits, with_std, place, st);
        if (rc != HM_OK) return rc;
    }
    if (body < E) {                                        // tail: less than one group
        MergeK kt = k;
        kt.elem0 = body; kt.n_elems = E - body;
        const int rc = launch_u16_generic<OUT>(kt, bits, with_std, st);
        if (rc != HM_OK) return rc;
    }
    return hot_pass();                                     // stream-ordered after the streaming pass: it overwrites the affected elements
}

static int merge_u16_entry(const hm_merge_args* g_in, hm_rules::MergeEntry entry, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16,
                           int bit_depth, void* stream) {
    const hm_rules::U16Extra x{frames_u16, bit_depth, darks_u16};
    hm_rules::MergeCall call;
    const int rc = hm_rules::check_merge_call(g_in, entry, &x, call);
    if (rc != HM_OK || call.empty) return rc;
    if (g_describe) g_describe->f32 = call.f32out;
    return call.f32out ? merge_u16_launch<OUT_F32>(call, stream) : merge_u16_launch<OUT_F64>(call, stream);
}

// the dispatch above with launching switched off (hm_merge_describe's mechanism). Returns for NULL args before anything else is read - or written.
static int merge_u16_describe(const hm_merge_args* g, hm_rules::MergeEntry entry, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16,
                              int bit_depth, char* buf, int buf_len) {
    if (!buf || buf_len < 1 || !g) return HM_EINVAL;
    DescribeCtx ctx;
    g_describe = &ctx;
    const int rc = merge_u16_entry(g, entry, frames_u16, darks_u16, bit_depth, nullptr);
    g_describe = nullptr;
    snprintf(buf, static_cast<size_t>(buf_len), "%s", ctx.names.c_str());
    return rc;
}

}  // namespace hm

extern "C" int64_t hm_merge_u16_algorithmic_bytes(const hm_merge_args* g) { return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_U16); }

extern "C" int hm_merge_u16(const hm_merge_args* g, const uint16_t* const* frames_u16, int bit_depth, void* stream) {
    return hm::merge_u16_entry(g, hm_rules::ENTRY_U16, frames_u16, nullptr, bit_depth, stream);
}

extern "C" int hm_merge_u16_describe(const hm_merge_args* g, const uint16_t* const* frames_u16, int bit_depth, char* buf, int buf_len) {
    return hm::merge_u16_describe(g, hm_rules::ENTRY_U16, frames_u16, nullptr, bit_depth, buf, buf_len);
}

// hm_merge_u16 with uint16 dark maps: the same launches, then the hot-pixel pass of hm_merge_u16_hot.hip where a frame has a map
extern "C" int64_t hm_merge_u16_darks_algorithmic_bytes(const hm_merge_args* g, const uint16_t* const* darks_u16) {
    return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_U16_DARKS, darks_u16);
}

extern "C" int hm_merge_u16_darks(const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, int bit_depth, void* stream) {
    return hm::merge_u16_entry(g, hm_rules::ENTRY_U16_DARKS, frames_u16, darks_u16, bit_depth, stream);
}

extern "C" int hm_merge_u16_darks_describe(const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, int bit_depth,
                                           char* buf, int buf_len) {
    return hm::merge_u16_describe(g, hm_rules::ENTRY_U16_DARKS, frames_u16, darks_u16, bit_depth, buf, buf_len);
}
