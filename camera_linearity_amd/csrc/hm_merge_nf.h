// hm_merge_nf.h - the compile-time-N kernels of the fused merge (merge_u8_fast, merge_u8_fast_std, merge_u8_fast_std_lut, merge_u8_val3)
// and their launchers, down to launch_fast_nf<NF, OUT>: everything behind one frame count and output type. Nothing here is instantiated
// by including it: the hm_merge_nf_*.hip units each instantiate launch_fast_nf for a range of frame counts (HM_INSTANTIATE_NF at the
// end), so each kernel is compiled in exactly one unit. In a tuning build (-DHM_TUNE_NF=<N>) the variant matrix of that N lands in
// whichever unit holds it.
#pragma once
#include "hm_merge_host.h"

namespace hm {

// ------------------------------------------------------------------------------------------------
// fast kernel: uint8 frames, C == 3, compile-time N.
// ------------------------------------------------------------------------------------------------

// Work decomposition of the fast kernel (tools/membench2.hip and tools/mergelab.hip are the experiments
// behind it): a wave owns "groups" of U * 128 consecutive elements. In a 128-element sub-unit lane l
// handles elements 2l and 2l+1:
//   * input: one global_load_ushort per (frame, sub-unit), 128 contiguous bytes per wave instruction,
//     immediate offsets 128*s off one scalar base;
//   * output: lane l owns the 16 contiguous bytes of elements 2l, 2l+1, so every store instruction is
//     one fully contiguous 1 KB global_store_dwordx4 (nontemporal) - no cross-lane transposition.
//     (Store instructions must cover whole 128-byte lines: 4 elements per lane stored directly is a
//     32-byte-stride pattern that costs 146 us instead of 128 us for the traffic alone; transposing
//     through LDS fixed that but added 13 % to an LDS pipe that bank conflicts already fill.)
// All group-level address arithmetic is scalar (the group index is wave-uniform). All N*U loads of a
// group are issued before the first gather; PREFETCH issues the next group's loads first.
// Channel of element 2l + j of sub-unit s of group g: (g*U*128 + 128*s + 2l + j) % 3 = (2*(g*U + s + l) + j) % 3.
//
// FLAT / SUMW = flat-field epilogue / sum-of-weights output compiled in (separate instantiations: a runtime
// branch around the flat-field loads cost config 3 ~100 us).

#ifndef HM_FB
#define HM_FB 4
#endif
#ifndef HM_STD_FB
#define HM_STD_FB 2      // std kernel, pass 2: frames per scheduling bundle
#endif

#ifndef HM_FLAT_PREFETCH
#define HM_FLAT_PREFETCH 1   // flat-field operands fetched one group ahead, with the frame bytes
#endif
#ifndef HM_STD_EARLY
#define HM_STD_EARLY 1       // std + flat-field kernel: issue every std load of a sub-unit before pass 1 (N <= HM_PIN_NF). A/B on one
#endif                       // box (tools/ab3.sh, profiles/r02_ab_std1.log): config 3 890 -> 847 us; without the flat field it costs 10 %, so FLAT only
#ifndef HM_PIN_NF
#define HM_PIN_NF 8      // std kernel: above this N, pass 2 re-derives its per-frame addresses (registers)
#endif

// merge_u8_fast_std with the per-DN std table (merge_u8_fast_std_lut): sub-units per group, frames per pass-2 scheduling bundle and
// the occupancy target, chosen for THIS instantiation from the compiler's resource report
// (HM_LUT_U sits in hm_merge_host.h: the dispatcher sizes the call's body with it)
#ifndef HM_LUT_FB
#define HM_LUT_FB 2
#endif
#ifdef HM_LUT_WAVES
#define HM_LUT_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(HM_LUT_WAVES, HM_LUT_WAVES)))
#else
#define HM_LUT_WAVES_ATTR
#endif

#ifdef HM_WAVES          /* experiment knob (tools/build_alt.sh): ask the register allocator for this many waves per SIMD */
#define HM_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(HM_WAVES, HM_WAVES)))
#else
#define HM_WAVES_ATTR
#endif

// SD (hm_merge_std_f32): element type of the std frames - float: the lane's two stds are one 8-byte load, widened once in registers.
template <int NF, int U, int TAB, bool STD, bool PREFETCH, bool FLAT, bool SUMW, int BLOCK, int CH = 3, int OUT = OUT_F64, bool LUT = false, typename SD = double>
__device__ __forceinline__ void merge_u8_fast_body(const MergeK& a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    reset_hot_counters(a);
    static_assert(CH == 3 || (CH == 1 && STD && !SUMW), "monochrome: the std instantiations (with or without the flat field) only");
    static_assert(!LUT || STD, "the per-DN std table belongs to the std kernel");
    constexpr int C = CH;
    // frames up to which pass 2 keeps its per-frame state pinned / its std loads issued early (flat-field instantiations). With the
    // sum-of-weights output on top, N = 8 needed 168 VGPRs + 20 bytes of scratch per lane: that one shape takes the N > 8 form (152 VGPRs)
    constexpr int PIN_NF = SUMW ? HM_PIN_NF - 1 : HM_PIN_NF;
    constexpr uint32_t GROUP = U * kSub;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lane2 = lane * 2u;
    const uint32_t lane16 = lane * 16u;          // byte offset of the lane's two float64 (scalar base + 32-bit VGPR offset addressing)
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr uint32_t WPB = BLOCK / 64;
    const uint32_t n_groups = static_cast<uint32_t>(a.n_elems / GROUP);
    const uint32_t gstride = gridDim.x * WPB;

    uint32_t g = blockIdx.x * WPB + wave;                                   // wave-uniform
    uint32_t raw[NF][U];
    auto load_group = [&](uint32_t grp, uint32_t (&dst)[NF][U]) {
        const int64_t off = a.in_off + static_cast<int64_t>(grp) * GROUP;   // scalar
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const uint8_t* p = static_cast<const uint8_t*>(a.frame[i]) + off;
#pragma unroll
            for (int s = 0; s < U; ++s) dst[i][s] = ld_u16(p + kSub * s + lane2);
        }
    };
    // flat-field operands of a group (FLAT only): with HM_FLAT_PREFETCH they are fetched one group ahead, with the frame bytes
    // (three waves per SIMD do not hide a load issued at the top of the sub-unit that consumes it)
    uint32_t fl_dn[U];
    f64x2 fl_v[U], fl_s[U];
    auto load_flat = [&](uint32_t grp, uint32_t (&dn)[U], f64x2 (&v)[U], f64x2 (&sd)[U]) {
        const int64_t fb = static_cast<int64_t>(grp) * GROUP;               // scalar, relative to row0
#pragma unroll
        for (int s = 0; s < U; ++s) {
            if (a.flat_u8) dn[s] = ld_u16(a.flat_u8 + fb + kSub * s + lane2);
            else v[s] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(reinterpret_cast<const char*>(a.flat_f64 + fb + kSub * s) + lane16));
            if (STD) sd[s] = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(reinterpret_cast<const char*>(a.flat_std + fb + kSub * s) + lane16));
        }
    };
    constexpr bool FLAT_PF = FLAT && PREFETCH && HM_FLAT_PREFETCH;
    // the first group's HBM loads are in flight while the workgroup builds its LDS tables
    if (PREFETCH && g < n_groups) {
        load_group(g, raw);
        if constexpr (FLAT_PF) load_flat(g, fl_dn, fl_v, fl_s);
    }

    if constexpr (!STD) {
        fill_val_tables<TAB>(lds, a);
    } else {
        double2* t_wdw = reinterpret_cast<double2*>(lds);
        double2* t_gd = reinterpret_cast<double2*>(lds + 16 * 256);
        for (int i = threadIdx.x; i < 256; i += BLOCK) t_wdw[i] = double2{a.w_lut[i], a.dw_lut[i]};
        // LUT (hm_merge_std_table): the entry's second half is dg itself, icrf_diff * std (measurand.py:512) - the product the std-stream
        // form makes per element-frame from the same two operands, made once per (DN, c); the kernel then has no std loads at all
        for (int i = threadIdx.x; i < 256 * C; i += BLOCK) t_gd[i] = double2{a.icrf[i], LUT ? a.icrf_diff[i] * a.std_lut[i] : a.icrf_diff[i]};
    }
    // uint8 flat fields take only 256 values: {F = DN/255, 1/F**2} per DN in LDS saves two float64 divisions per element
    double2* t_flat = reinterpret_cast<double2*>(lds + (STD ? kStdTabBytes : TabInfo<TAB>::bytes));
    if constexpr (FLAT) {
        for (int i = threadIdx.x; i < 256; i += BLOCK) {
            const double F = static_cast<double>(i) / 255.0;
            t_flat[i] = double2{F, 1.0 / (F * F)};
        }
    }
    __syncthreads();

    for (; g < n_groups; g += gstride) {
        uint32_t cur[NF][U];
        uint32_t cfl_dn[U];
        f64x2 cfl_v[U], cfl_s[U];
        if constexpr (PREFETCH) {
#pragma unroll
            for (int i = 0; i < NF; ++i)
#pragma unroll
                for (int s = 0; s < U; ++s) cur[i][s] = raw[i][s];
            if constexpr (FLAT_PF) {
#pragma unroll
                for (int s = 0; s < U; ++s) { cfl_dn[s] = fl_dn[s]; cfl_v[s] = fl_v[s]; cfl_s[s] = fl_s[s]; }
            }
            if (g + gstride < n_groups) {
                load_group(g + gstride, raw);
                if constexpr (FLAT_PF) load_flat(g + gstride, fl_dn, fl_v, fl_s);
            }
        } else {
            load_group(g, cur);
        }
        if constexpr (FLAT && !FLAT_PF) load_flat(g, cfl_dn, cfl_v, cfl_s);
        const int64_t gbase = static_cast<int64_t>(g) * GROUP;            // relative to row0, scalar

#pragma unroll
        for (int s = 0; s < U; ++s) {
            const int64_t sbase = gbase + kSub * s;                         // scalar
            const uint32_t c0 = C == 1 ? 0u : (2u * (g * U + s + lane)) % 3u;
            const uint32_t c1 = C == 1 ? 0u : (c0 + 1u) % 3u;
            const uint32_t coffs[2] = {STD ? c0 * 16u : chan_off<TAB>(c0), STD ? c1 * 16u : chan_off<TAB>(c1)};
            double* ov = out_at<OUT>(a.out_val, sbase);                       // scalar bases
            double* osw = SUMW ? a.out_sum_w + sbase : nullptr;

            // flat-field operands of the lane's two elements (one ushort / 16-byte loads)
            double F[2] = {1.0, 1.0}, sF[2] = {0.0, 0.0}, iF2[2] = {1.0, 1.0};
            if constexpr (FLAT) {
                {
                    if (a.flat_u8) {
                        const uint32_t f = cfl_dn[s];
                        const double2 f0 = t_flat[f & 255u], f1 = t_flat[f >> 8];
                        F[0] = f0.x; iF2[0] = f0.y; F[1] = f1.x; iF2[1] = f1.y;
                    } else {
                        const f64x2 f = cfl_v[s];
                        F[0] = f.x; F[1] = f.y;
                        if (STD) { iF2[0] = 1.0 / (F[0] * F[0]); iF2[1] = 1.0 / (F[1] * F[1]); }
                    }
                    if (STD) { sF[0] = cfl_s[s].x; sF[1] = cfl_s[s].y; }
                }
            }

            if constexpr (!STD) {
                double S[2], acc[2];
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    const double it = a.inv_t[i];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const uint32_t dn = j == 0 ? (cur[i][s] & 255u) : (cur[i][s] >> 8);
                        double w, wg;
                        gather_val<TAB>(lds, dn, coffs[j], w, wg);
                        if (i == 0) { S[j] = w; acc[j] = wg * it; }
                        else {
                            S[j] += w;                               // exposure_series.py:340
                            acc[j] = fma(wg, it, acc[j]);            // :388 numerator
                        }
                    }
                    // bound the gathers in flight (HM_FB frames = 2*HM_FB ds_read_b128, 8*HM_FB VGPRs) per scheduling
                    // bundle; HM_FB = 4 measured best (2: more VGPRs and 144 us; none: everything hoisted)
                    if (((i % HM_FB) == HM_FB - 1 || i == NF - 1)) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) { HM_PIN(S[j]); HM_PIN(acc[j]); }
                        __builtin_amdgcn_sched_barrier(0);
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
                if constexpr (SUMW) store2(osw, lane16, S[0], S[1]);
                store_pair<OUT>(ov, lane16, val[0], val[1]);
            } else {
                const double2* t_wdw = reinterpret_cast<const double2*>(lds);
                const char* t_gd = lds + 16 * 256;
                // HM_STD_EARLY (flat-field instantiations): all NF float64 std loads of the sub-unit are issued here, ahead of pass 1's
                // gathers (4 VGPRs per frame: stacks of up to HM_PIN_NF frames only), instead of HM_STD_FB frames at a time inside pass 2
                constexpr bool EARLY = !LUT && HM_STD_EARLY && FLAT && NF <= PIN_NF;
                typename SdPair<SD>::type sd_early[EARLY ? NF : 1];
                if constexpr (EARLY) {
#pragma unroll
                    for (int i = 0; i < NF; ++i) sd_early[i] = ld_sd_pair_global<SD>(a.template sd_as<SD>(i) + a.in_off + sbase, lane16);
                }
                // pass 1: S = sum_i w_i
                double S[2];
#pragma unroll
                for (int i = 0; i < NF; ++i) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
#ifdef HM_PROBE_STD   /* table-free traffic probe of the std kernels (wrong results; tuning builds only) */
                        const double w = static_cast<double>((j == 0 ? (cur[i][s] & 255u) : (cur[i][s] >> 8)) + 1u);
#else
                        const double w = t_wdw[j == 0 ? (cur[i][s] & 255u) : (cur[i][s] >> 8)].x;
#endif
                        if (i == 0) S[j] = w; else S[j] += w;
                    }
                    if ((i & 3) == 3 && i != NF - 1) {      // at most 8 weight gathers in flight (large N: registers)
                        HM_PIN(S[0]); HM_PIN(S[1]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                double invS[2], invS2[2], acc[2], var[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    invS[j] = 1.0 / S[j];
                    invS2[j] = 1.0 / (S[j] * S[j]);                  // 1 / S**2, exposure_series.py:343
                    HM_PIN(invS[j]); HM_PIN(invS2[j]);
                }
                __builtin_amdgcn_sched_barrier(0);
                // pass 2
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    const double it = a.inv_t[i];
                    typename SdPair<SD>::type sdv;
                    if constexpr (LUT) sdv = typename SdPair<SD>::type{1.0, 1.0};   // unused: the table entry is dg
                    else if constexpr (EARLY) sdv = sd_early[i];
                    else {
                        const SD* sp = a.template sd_as<SD>(i) + a.in_off + sbase;               // scalar base
                        if (NF > PIN_NF || !FLAT) asm volatile("" : "+s"(sp));     // keep base + 32-bit lane offset addressing (no per-frame VGPR address pairs)
                        sdv = ld_sd_pair_global<SD>(sp, lane16);
                    }
                    uint32_t packed = cur[i][s];
                    if (LUT || NF > PIN_NF || !FLAT) HM_PIN(packed);           // re-extract the DNs here instead of keeping pass 1's indices alive
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const uint32_t dn = j == 0 ? (packed & 255u) : (packed >> 8);
#ifdef HM_PROBE_STD
                        const double2 wdw = double2{static_cast<double>(dn + 1u), static_cast<double>(dn + 2u)};
                        const double2 gd = double2{static_cast<double>(dn + coffs[j]), static_cast<double>(dn + 3u)};
#else
                        const double2 wdw = t_wdw[dn];
                        const double2 gd = *reinterpret_cast<const double2*>(t_gd + dn * (16u * C) + coffs[j]);
#endif
                        const double w = wdw.x, dw = wdw.y, gg = gd.x;
                        const double dg = LUT ? gd.y : gd.y * static_cast<double>(j == 0 ? sdv.x : sdv.y);   // measurand.py:512
                        // merge_var_term() of hm_merge_math.h, written out: called here, the N = 1 kernels schedule differently
                        const double A = (dw * gg + w * dg) * invS[j] - ((dw * w) * gg) * invS2[j];   // :389
                        const double term = (A * dg) * it;
                        if (i == 0) { acc[j] = (w * gg) * it; var[j] = term * term; }
                        else {
                            acc[j] = fma(w * gg, it, acc[j]);                                    // :388
                            var[j] = fma(term, term, var[j]);
                        }
                    }
                    constexpr int FB = LUT ? HM_LUT_FB : HM_STD_FB;
                    if ((i % FB) == FB - 1 || i == NF - 1) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) { HM_PIN(acc[j]); HM_PIN(var[j]); }
                        __builtin_amdgcn_sched_barrier(0);   // FB frames' std loads + gathers at a time
                    }
                }
                double val[2], so[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    val[j] = acc[j] / S[j];
                    so[j] = sqrt(var[j]);                                                        // :394
                }
                if constexpr (FLAT) {
                    flat_field_math(F[0], iF2[0], sF[0], a.ff_mean[c0], a.ff_std_mean[c0], true, val[0], so[0]);
                    flat_field_math(F[1], iF2[1], sF[1], a.ff_mean[c1], a.ff_std_mean[c1], true, val[1], so[1]);
                }
                if constexpr (SUMW) store2(osw, lane16, S[0], S[1]);
                store_pair<OUT>(ov, lane16, val[0], val[1]);
                store_pair<OUT>(out_at<OUT>(a.out_std, sbase), lane16, so[0], so[1]);
            }
            __builtin_amdgcn_sched_barrier(0);   // keep one sub-unit's gathers from piling onto the next one's
        }
    }
}

// Entry points. The std kernel is given an occupancy target of 3 waves/SIMD: with up to 168 VGPRs the scheduler keeps more
// loads in flight per wave (A/B on one box, tools/ab3.sh: 7 x 4096 x 4096 x 3 + std 716 -> 697 us, + flat field 869 -> 823 us;
// targets 4 and 5 are slower, the val-only kernel is insensitive).
#ifndef HM_STD_WAVES
#define HM_STD_WAVES 3
#endif
// Round 4: the flat-field instantiations (two more streams, the early std loads, the epilogue's operands) take a target of 2: config 3's
// std + flat stack 808-821 -> 790-792 us on one box, two runs each (tools/gpu_r04f.sh, profiles/r04f_*); without a flat field 2 costs 7 %.
#ifndef HM_STD_WAVES_FLAT
#define HM_STD_WAVES_FLAT 2
#endif
template <int NF, int U, int TAB, bool STD, bool PREFETCH, bool FLAT, bool SUMW, int BLOCK, int OUT = OUT_F64>
__global__ __launch_bounds__(BLOCK) HM_WAVES_ATTR void merge_u8_fast(const MergeK a) {
    static_assert(!STD, "std instantiations go through merge_u8_fast_std");
    merge_u8_fast_body<NF, U, TAB, false, PREFETCH, FLAT, SUMW, BLOCK, 3, OUT>(a);
}
template <int NF, int U, int TAB, bool PREFETCH, bool FLAT, bool SUMW, int BLOCK, int CH = 3, int OUT = OUT_F64, typename SD = double>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(FLAT ? HM_STD_WAVES_FLAT : HM_STD_WAVES, FLAT ? HM_STD_WAVES_FLAT : HM_STD_WAVES)))
void merge_u8_fast_std(const MergeK a) {
    merge_u8_fast_body<NF, U, TAB, true, PREFETCH, FLAT, SUMW, BLOCK, CH, OUT, false, SD>(a);
}
// The same kernel with the per-DN std table (hm_merge_std_table): no std loads, the {g, dg} entries carry the table. Its register
// budget is its own (HM_LUT_U / HM_LUT_FB / HM_LUT_WAVES below), not the std-stream kernel's.
template <int NF, int U, bool FLAT, int OUT = OUT_F64>
__global__ __launch_bounds__(256) HM_LUT_WAVES_ATTR void merge_u8_fast_std_lut(const MergeK a) {
    merge_u8_fast_body<NF, U, TAB_PLAIN, true, true, FLAT, false, 256, 3, OUT, true>(a);
}

// ------------------------------------------------------------------------------------------------
// merge_u8_val3: val-only merge of uint8 frames, C == 3, compile-time N, no extras - the bench kernel (config 2).
//
// Element -> lane ownership is that of merge_u8_fast (lane l owns elements 2l, 2l+1 of a 128-element sub-unit: one
// global_load_ushort per frame, one fully contiguous 1 KB global_store_dwordx4 per wave), what changes is everything
// around the gathers, which rocprof showed to be the larger part of the VALU stream (profiles/r01g: 7.9 VALU
// instructions per element-frame, 2 of them the float64 accumulation):
//   * a wave's group is THREE sub-units = 384 elements = 128 whole pixels, so every group starts on channel 0 and the
//     channel of element j of sub-unit s is (2s + 2l + j) % 3 - a compile-time function of (s, j) on top of the lane
//     constant (2l) % 3. The three possible table offsets live in three VGPRs for the whole kernel; merge_u8_fast
//     recomputed its channel offsets per sub-unit with 32-bit multiplies-high (% 3 of a run-time group index).
//     The LDS address of a gather is then one v_mad_u32_u24 (dn * 48 + offset) after the byte extraction.
//   * the next group's loads go into a second register set and the loop body is written out twice (A/B), so the
//     prefetch costs no register-to-register copies (14 v_mov per 256 elements before).
//   * acc / S uses the correctly rounded reciprocal-Newton-Markstein sequence WITHOUT the operand scaling and fix-up
//     steps of the IEEE division expansion (v_div_scale x2, v_div_fixup: 3 of its 11 instructions) whenever the
//     workgroup has proven, while building its tables, that no operand can leave the range in which those steps are
//     the identity (div_inrange below); otherwise the plain division. Both give the same bits.
// ------------------------------------------------------------------------------------------------

// a / b, correctly rounded, for operands in the range the table check guarantees: b in [2^-64, 2^70] and a either +0 or
// |a| in [2^-660, 2^610]. This is instruction for instruction what hipcc emits for a float64 division minus the two
// v_div_scale_f64 (which return their operands unchanged in that range: no operand is denormal, the quotient and 1/b
// are normal, the numerator's biased exponent is above 53 and the exponent difference below 768) and the
// v_div_fixup_f64 (which only rewrites zero / infinite / NaN cases): r = rcp(b) refined twice, q = a r,
// q' = q + (a - b q) r (Markstein). a = +0 gives +0 on both paths; -0 never reaches it (the check rejects tables that hold one).
__device__ __forceinline__ double div_inrange(double a, double b) {
    double r = __builtin_amdgcn_rcp(b);
    double e = fma(-b, r, 1.0);
    r = fma(r, e, r);
    e = fma(-b, r, 1.0);
    r = fma(r, e, r);
    const double q = a * r;
    const double res = fma(-b, q, a);
    return fma(res, r, q);
}
template <bool FASTDIV>
__device__ __forceinline__ double merge_div(double a, double b) {
    if constexpr (FASTDIV) return div_inrange(a, b);
    else return a / b;
}
// table entry check behind div_inrange: w in [2^-64, 2^64]; w*g either +0 (bit pattern) or in [2^-300, 2^300] - POSITIVE: with
// entries of both signs the fma chain could cancel far below any single term (down to ~2^-706 for 16 frames), outside the range the
// argument above covers. Non-negative terms only grow the sum: acc is +0 or in [2^-600, 2^605] (times 1/t in [2^-300, 2^300], 16 terms).
__device__ __forceinline__ bool entry_inrange(double w, double wg) {
    const bool w_ok = w >= 0x1p-64 && w <= 0x1p64;
    const bool wg_ok = __double_as_longlong(wg) == 0 || (wg >= 0x1p-300 && wg <= 0x1p300);
    return w_ok && wg_ok;
}

// Template parameters (the defaults are chosen by launch_val3(); the others exist for A/B runs, tools/ab_val3.py):
//   U    sub-units of 128 elements per wave and iteration (2 or 3).
//   PF   0: in-place refill - each R register is reloaded with the next unit's bytes as soon as its DNs have been turned
//           into LDS addresses (one register set, loads issued in bundles of HM_FB frames between the gathers);
//        1: the next unit's loads are all issued at the top of the iteration into a second register set (A/B ping-pong).
//   MAP  0: a wave owns U*128 contiguous elements per iteration ("group");
//        1: the WORKGROUP owns U*512 contiguous elements ("chunk") and slot s of wave w sits at 512 s + 128 w, so the four
//           waves' loads of one time slot cover 512 contiguous bytes of every frame and their stores 4 contiguous KB.
// A unit (group or chunk) must start on channel 0 for the channel pattern to be a compile-time function of (s, j): its
// size is a multiple of 3 when U == 3; for U == 2 the unit index advances by a multiple of 3 per iteration (the host
// launches a multiple of 3 workgroups), so the phase is a per-wave constant folded into the lane's table offsets.
// FLAT (round 3; uint8 flat fields, PF == 1): the val-only flat-field epilogue (val / F) * m of measurand.py:602 - the flat's DNs travel as
// one more byte stream beside the frames', F = DN / 255 comes from a 2 KB LDS table, the channel means sit in three registers next to
// the table offsets. Before, a flat field sent the val-only merge to merge_u8_fast (186 us / 0.54 on config 2's stack).
// CH (round 3): 3 = colour (the channel pattern above), 1 = monochrome cameras - one table column, no channel bookkeeping at all; before,
// every C != 3 stack went to the run-time-N, run-time-C merge_u8_loop (0.62-0.68 val-only on 7 x 4096 x 4096 x 1).
#ifndef HM_VAL3_PROBE
#define HM_VAL3_PROBE 0      // measurement builds only (wrong results): 1 = no LDS gathers (the ceiling of the HBM access pattern); 2 = every unit's
#endif                       // frame bytes come from the first 64 units (L2 hits; the gathers and the stores are real); 3 = 2 without the stores
// OUT / QUAD (float32 outputs): OUT_F32 stores float32 elements. With the pair map above that is 8 bytes per lane and store instruction,
// half of what the float64 form moves per instruction. QUAD (OUT_F32, PF == 1, even U, MAP 0 or 3) keeps 16-byte stores by changing the
// element map instead of exchanging values between lanes: lane l owns FOUR consecutive elements 4l .. 4l+3 of a 256-element span - one
// global_load_dword per frame and span (half as many load instructions, half as many byte registers) and one contiguous 1 KB
// global_store_dwordx4 per wave and span. "Slot" s of the pair map becomes half a span: s even = elements 4l, 4l+1, s odd = 4l+2, 4l+3 of span
// s / 2, and the channel of element j of slot s is (4l + (s / 2) + 2 (s % 2) + j) % 3 - still a compile-time function of (s, j) on top of a lane
// constant. The arithmetic per element is untouched. Needs the frames (and the flat field) 4-byte aligned at the call's first element and
// the output 16-byte aligned; hm_merge sends other calls to the pair form (DESIGN.md 4.1.1 has the measured pair).
#if HM_VAL3_PROBE >= 2
#define HM_PROBE_UNIT(x) ((x) & 63u)
#else
#define HM_PROBE_UNIT(x) (x)
#endif
template <int NF, int U, int PF, int MAP, bool FLAT = false, int CH = 3, int OUT = OUT_F64, bool QUAD = false>
__global__ __launch_bounds__(256) void merge_u8_val3(const MergeK a) {
    static_assert(CH == 3 || CH == 1, "colour or monochrome");
    static_assert(!QUAD || (OUT == OUT_F32 && PF == 1 && U % 2 == 0 && (MAP == 0 || MAP == 3)), "the four-elements-per-lane map: float32 outputs, prefetch form, whole spans");
    constexpr uint32_t TS = 16u * CH;                              // bytes of table per DN
    __shared__ __attribute__((aligned(16))) char lds[16 * 256 * CH];
    __shared__ uint32_t s_bad[4];
    __shared__ double t_F[FLAT ? 256 : 1];
    static_assert(!FLAT || PF == 1, "the flat-field instantiation uses the two-register-set prefetch");
    constexpr int NS = NF + (FLAT ? 1 : 0);                        // byte streams: the frames (+ the flat field's DNs as stream NF)
    reset_hot_counters(a);
    constexpr bool DEFER = MAP == 2;                               // MAP 2: the element map of MAP 0, all U stores of a unit issued together at its end
    constexpr bool PIPE = MAP == 3;                                // MAP 3: the element map of MAP 0, the gathers of frame bundle b + 1 issued under the accumulation of bundle b
    constexpr bool WGMAP = MAP == 1;
    constexpr uint32_t SLOT = WGMAP ? 4u * kSub : kSub;            // element distance between a wave's consecutive slots
    constexpr uint32_t UNIT = U * SLOT;                            // elements per unit (group: U*128, chunk: U*512)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lane16 = lane * 16u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wave_el = WGMAP ? wave * kSub : 0u;             // scalar: the wave's element offset inside a chunk
    const uint32_t lane2 = QUAD ? lane * 4u : lane * 2u + wave_el; // element (= byte) offset of the lane's first element inside the unit
    constexpr int UR = QUAD ? U / 2 : U;                           // byte registers per frame and unit (QUAD: one dword per 256-element span)
    constexpr uint32_t RSLOT = QUAD ? 2u * SLOT : SLOT;            // element distance between them
    const uint32_t n_units = static_cast<uint32_t>(a.n_elems / UNIT);
    const uint32_t ustride = WGMAP ? gridDim.x : gridDim.x * 4u;
    uint32_t u = WGMAP ? blockIdx.x : blockIdx.x * 4u + wave;      // wave-uniform

    // R[i][s]: the two DNs of frame i, slot s (kept 16-bit: widening at the load would put a v_and - and a wait for the
    // load - right behind it)
    // (PF == 1 keeps 32-bit registers filled by zero-extending global loads: with two 16-bit register sets hipcc packs pairs
    // of them into one VGPR with v_perm_b32 at the loop back-edge, i.e. waits for the prefetch it has just issued)
    using reg_t = std::conditional_t<PF == 0, uint16_t, uint32_t>;
    reg_t RA[NS][UR], RB[PF ? NS : 1][PF ? UR : 1];
    auto ld_reg = [](const uint8_t* q) { if constexpr (QUAD) return ld_u32(q); else return ld_u16(q); };
    // the two DNs of frame i, slot s (QUAD: the low / high half of the span's dword)
    auto dn_pair = [](const auto& regs, int i, int s_) {
        if constexpr (QUAD) return (s_ & 1) ? (regs[i][s_ >> 1] >> 16) : (regs[i][s_ >> 1] & 0xffffu);
        else return regs[i][s_];
    };
    // element j of slot s, counted from the lane's first element, modulo 3
    auto el = [](int s_, int j) constexpr { return QUAD ? (s_ / 2) + 2 * (s_ % 2) + j : 2 * s_ + j; };
    auto load_unit = [&](uint32_t unit, auto& dst) {
        if constexpr (FLAT) {                                      // the flat field covers the OUTPUT rows: no in_off
            const uint8_t* p = a.flat_u8 + static_cast<int64_t>(unit) * UNIT;
#pragma unroll
            for (int s = 0; s < UR; ++s) dst[NF][s] = ld_reg(p + RSLOT * s + lane2);
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            if constexpr (PF == 0) {
                const __amdgpu_buffer_rsrc_t fr = frame_rsrc(static_cast<const uint8_t*>(a.frame[i]) + a.in_off);
#pragma unroll
                for (int s = 0; s < U; ++s) dst[i][s] = ld_u16_buf(fr, lane2 + SLOT * s, HM_PROBE_UNIT(unit) * UNIT);
            } else {
                const uint8_t* p = static_cast<const uint8_t*>(a.frame[i]) + a.in_off + static_cast<int64_t>(HM_PROBE_UNIT(unit)) * UNIT;
#pragma unroll
                for (int s = 0; s < UR; ++s) dst[i][s] = ld_reg(p + RSLOT * s + lane2);
            }
        }
    };
    if (u < n_units) load_unit(u, RA);                                              // in flight while the tables are built

    bool bad = false;
    for (int q = threadIdx.x; q < 256 * CH; q += 256) {
        const double w = a.w_lut[q / CH];
        const double wg = w * a.icrf[q];                                            // (w * g), exposure_series.py:388
        reinterpret_cast<double2*>(lds)[q] = double2{w, wg};
        bad = bad || !entry_inrange(w, wg);
    }
    if constexpr (FLAT) t_F[threadIdx.x] = static_cast<double>(threadIdx.x) / 255.0;     // F = DN / 255 (image_set.py:223)
    const bool wave_bad = __ballot(bad) != 0ull;
    if (lane == 0) s_bad[wave] = wave_bad ? 1u : 0u;
    __syncthreads();
    const uint32_t any_bad = __builtin_amdgcn_readfirstlane(s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]);
    const bool fastdiv = any_bad == 0u && a.inv_t_inrange != 0;                     // scalar
    if (u >= n_units) return;

    // channel of the lane's first element in slot 0: (unit start + wave offset + 2 lane) % 3; the unit start is a
    // per-wave constant mod 3 (see above)
    const uint32_t p0 = CH == 1 ? 0u : static_cast<uint32_t>((static_cast<uint64_t>(u) * UNIT) % 3u);
    const uint32_t k = CH == 1 ? 0u : (p0 + lane2) % 3u;
    const uint32_t off[3] = {k * 16u, CH == 1 ? 0u : ((k + 1u) % 3u) * 16u, CH == 1 ? 0u : ((k + 2u) % 3u) * 16u};
    auto ci = [](int x) constexpr { return CH == 1 ? 0 : x % 3; };      // which of the three offsets / means element x of a unit uses
    // FLAT: the ROI means of the channels k, k + 1, k + 2 (no per-lane indexing of the kernarg array)
    double mm[3] = {1.0, 1.0, 1.0};
    if constexpr (FLAT) {
        const double m0 = a.ff_mean[0], m1 = CH == 1 ? m0 : a.ff_mean[1], m2 = CH == 1 ? m0 : a.ff_mean[2];
        mm[0] = k == 0u ? m0 : k == 1u ? m1 : m2;
        mm[1] = k == 0u ? m1 : k == 1u ? m2 : m0;
        mm[2] = k == 0u ? m2 : k == 1u ? m0 : m1;
    }
    auto flat_epilogue = [&](int s_, uint32_t r, double& v0, double& v1) {          // measurand.py:602, as flat_field_math() does it
        if constexpr (FLAT) {
            v0 = (v0 / t_F[r & 255u]) * mm[ci(el(s_, 0))];
            v1 = (v1 / t_F[r >> 8]) * mm[ci(el(s_, 1))];
        }
    };

    // one unit out of `cur`; REFILL (PF == 0 only): fetch the next unit's bytes into the registers this one frees
    auto process = [&](auto refill_tag, uint32_t unit, auto& cur) {
        constexpr bool REFILL = decltype(refill_tag)::value;
        const uint32_t next_off = HM_PROBE_UNIT(unit + ustride) * UNIT;                                   // scalar: byte offset of the next unit in every frame
        double* og = out_at<OUT>(a.out_val, static_cast<int64_t>(unit) * UNIT + wave_el);    // scalar base of the wave's output in this unit
        double held[DEFER ? U : 1][2];
        // the slot's two results: stored as a pair, or (QUAD) the even slot's kept as two floats until the odd slot completes the lane's four
        float q0 = 0.0f, q1 = 0.0f;
        auto emit = [&](int s_, double v0, double v1) {
            if constexpr (QUAD) {
                if (s_ % 2 == 0) { q0 = static_cast<float>(v0); q1 = static_cast<float>(v1); }
                else store_quad_f32(out_at<OUT>(og, RSLOT * (s_ / 2)), lane16, q0, q1, static_cast<float>(v0), static_cast<float>(v1));
            } else {
                store_pair<OUT>(out_at<OUT>(og, SLOT * s_), lane16, v0, v1);
            }
        };
        if constexpr (PIPE) {
            // software-pipelined gathers ("software-pipelined LDS gathers"): two sets of gathered {w, w g} pairs; the ds_read_b128 of the next
            // bundle of HM_FB frames (of this or the next sub-unit) are in flight while the current bundle's add / fma chain runs
            constexpr int NB = (NF + HM_FB - 1) / HM_FB;
            double2 T[2][HM_FB][2];
            auto issue = [&](int s_, int b_, double2 (&dst)[HM_FB][2]) {
#pragma unroll
                for (int f = 0; f < HM_FB; ++f) {
                    if (b_ * HM_FB + f < NF) {
                        const auto r = dn_pair(cur, b_ * HM_FB + f, s_);
                        dst[f][0] = *reinterpret_cast<const double2*>(lds + (__umul24(static_cast<uint32_t>(r & 255u), TS) + off[ci(el(s_, 0))]));
                        dst[f][1] = *reinterpret_cast<const double2*>(lds + (__umul24(static_cast<uint32_t>(r >> 8), TS) + off[ci(el(s_, 1))]));
                    }
                }
                if constexpr (REFILL) {                     // PF == 0: the bytes just turned into addresses make room for the next unit's
#pragma unroll
                    for (int f = 0; f < HM_FB; ++f)
                        if (b_ * HM_FB + f < NF)
                            cur[b_ * HM_FB + f][s_] = ld_u16_buf(frame_rsrc(static_cast<const uint8_t*>(a.frame[b_ * HM_FB + f]) + a.in_off), lane2 + SLOT * s_, next_off);
                }
            };
            issue(0, 0, T[0]);
#pragma unroll
            for (int s = 0; s < U; ++s) {
                double S[2], acc[2];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    constexpr int dummy = 0; (void)dummy;
                    const int gi = s * NB + b;
                    if (gi + 1 < U * NB) issue((gi + 1) / NB, (gi + 1) % NB, T[(gi + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int f = 0; f < HM_FB; ++f) {
                        if (b * HM_FB + f < NF) {
                            const double it = a.inv_t[b * HM_FB + f];
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                const double2 t = T[gi & 1][f][j];
                                if (b * HM_FB + f == 0) { S[j] = t.x; acc[j] = t.y * it; }
                                else {
                                    S[j] += t.x;                               // exposure_series.py:340
                                    acc[j] = fma(t.y, it, acc[j]);             // :388 numerator
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) { HM_PIN(S[j]); HM_PIN(acc[j]); }
                    __builtin_amdgcn_sched_barrier(0);
                }
                double v0, v1;
                if (fastdiv) { v0 = div_inrange(acc[0], S[0]); v1 = div_inrange(acc[1], S[1]); }
                else { v0 = acc[0] / S[0]; v1 = acc[1] / S[1]; }
                flat_epilogue(s, dn_pair(cur, NS - 1, s), v0, v1);
                emit(s, v0, v1);
                __builtin_amdgcn_sched_barrier(0);
            }
            return;
        }
#pragma unroll
        for (int s = 0; s < U; ++s) {
            double S[2], acc[2];
#pragma unroll
            for (int i0 = 0; i0 < NF; i0 += HM_FB) {                                // HM_FB frames per scheduling bundle
                uint32_t addr[HM_FB][2];
#pragma unroll
                for (int f = 0; f < HM_FB; ++f) {
                    if (i0 + f < NF) {
                        const auto r = dn_pair(cur, i0 + f, s);
                        addr[f][0] = __umul24(static_cast<uint32_t>(r & 255u), TS) + off[ci(el(s, 0))];
                        addr[f][1] = __umul24(static_cast<uint32_t>(r >> 8), TS) + off[ci(el(s, 1))];
                    }
                }
                if constexpr (REFILL) {
                    __builtin_amdgcn_sched_barrier(0);      // the refill must not be hoisted above the last use of the old bytes (it would need a second register set)
#pragma unroll
                    for (int f = 0; f < HM_FB; ++f)
                        if (i0 + f < NF)
                            cur[i0 + f][s] = ld_u16_buf(frame_rsrc(static_cast<const uint8_t*>(a.frame[i0 + f]) + a.in_off), lane2 + SLOT * s, next_off);
                }
#pragma unroll
                for (int f = 0; f < HM_FB; ++f) {
                    if (i0 + f < NF) {
                        const double it = a.inv_t[i0 + f];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
#if HM_VAL3_PROBE == 1
                            const double2 t = double2{static_cast<double>(addr[f][j] + 1u), static_cast<double>(addr[f][j])};
#else
                            const double2 t = *reinterpret_cast<const double2*>(lds + addr[f][j]);
#endif
                            if (i0 + f == 0) { S[j] = t.x; acc[j] = t.y * it; }
                            else {
                                S[j] += t.x;                               // exposure_series.py:340
                                acc[j] = fma(t.y, it, acc[j]);             // :388 numerator
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) { HM_PIN(S[j]); HM_PIN(acc[j]); }
                __builtin_amdgcn_sched_barrier(0);
            }
            double v0, v1;
            if (fastdiv) { v0 = div_inrange(acc[0], S[0]); v1 = div_inrange(acc[1], S[1]); }
            else { v0 = acc[0] / S[0]; v1 = acc[1] / S[1]; }
            flat_epilogue(s, dn_pair(cur, NS - 1, s), v0, v1);
            if constexpr (DEFER) { held[s][0] = v0; held[s][1] = v1; }
#if HM_VAL3_PROBE == 3
            else { if (v0 != v0 && v1 == 12345.0) store_pair<OUT>(out_at<OUT>(og, SLOT * s), lane16, v0, v1); }
#else
            else emit(s, v0, v1);
#endif
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (DEFER) {                      // U KB of contiguous output in U back-to-back store instructions
#pragma unroll
            for (int s = 0; s < U; ++s) store_pair<OUT>(out_at<OUT>(og, SLOT * s), lane16, held[s][0], held[s][1]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if constexpr (PF == 0) {
        for (; u + ustride < n_units; u += ustride) process(std::true_type{}, u, RA);
        process(std::false_type{}, u, RA);
    } else {
        while (true) {                                                               // RA holds unit u
            if (u + ustride >= n_units) { process(std::false_type{}, u, RA); break; }
            load_unit(u + ustride, RB);
            __builtin_amdgcn_sched_barrier(0);
            process(std::false_type{}, u, RA);
            u += ustride;                                                            // RB holds unit u
            if (u + ustride >= n_units) { process(std::false_type{}, u, RB); break; }
            load_unit(u + ustride, RA);
            __builtin_amdgcn_sched_barrier(0);
            process(std::false_type{}, u, RB);
            u += ustride;
        }
    }
}

#if HM_TUNE_NF != 0
#include "../../tools/hm_merge_priv.inc"     // merge_u8_priv: the conflict-free-LDS experiment (tuning builds only, lives with the other experiments)
#endif

// ------------------------------------------------------------------------------------------------
// host side: the launchers of the kernels above
// ------------------------------------------------------------------------------------------------
template <int NF, int U, int TAB, bool STD, bool PF, bool FLAT, bool SUMW, int BLOCK, int CH = 3, int OUT = OUT_F64, typename SD = double>
static int launch_one(const MergeK& k, hipStream_t st) {
    constexpr int lds = (STD ? kStdTabBytes : TabInfo<TAB>::bytes) + (FLAT ? 16 * 256 : 0);
    void (*kernel)(const MergeK);
    if constexpr (STD) kernel = merge_u8_fast_std<NF, U, TAB, PF, FLAT, SUMW, BLOCK, CH, OUT, SD>;
    else kernel = merge_u8_fast<NF, U, TAB, false, PF, FLAT, SUMW, BLOCK, OUT>;
    if (describe_only(CH == 1 ? "merge_u8_fast_std<N=%d,U=%d,flat=%d,sum_w=%d,C=1>"
                              : (STD ? "merge_u8_fast_std<N=%d,U=%d,flat=%d,sum_w=%d>" : "merge_u8_fast<N=%d,U=%d,flat=%d,sum_w=%d>"), NF, U, FLAT, SUMW)) return HM_OK;
    int per_cu = 2048 / BLOCK;                       // 32 waves per CU
    if (kMaxLds / lds < per_cu) per_cu = kMaxLds / lds;
    if (const int e = tune_env("HM_TUNE_WG_PER_CU", 1, 64)) per_cu = e;
    const int64_t groups = k.n_elems / (U * static_cast<int>(kSub));
    const unsigned grid = stream_grid(groups, BLOCK / 64, per_cu);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), lds, st, k);
    return launch_status();
}

template <int NF, int U, int PF, int MAP, bool FLAT = false, int CH = 3, int OUT = OUT_F64, bool QUAD = false>
static int launch_val3_cfg(const MergeK& k, hipStream_t st) {
    const int64_t units = k.n_elems / (U * (MAP == 1 ? 4 : 1) * static_cast<int>(kSub));
    // workgroups per CU (8 are resident). U = 2 (N <= 8): 12 - a grid of 3072 is a multiple of 3 as it stands (2048 had to become 2046) and
    // config 2's 196 608 units divide evenly among its waves; same-process A/B with shared output buffers (tools/ab_val3.py, variants
    // W * 10000 + 7210 of a tuning build, profiles/r02h_ab_val3_wg_per_cu.log): 134.9 against 136.7 us (8) on a slow box, 129.0 against 129.9 us
    // on a fast one; 2, 3, 4, 6, 16, 24, 32 are no better. U = 3 keeps 8 (config 4's tile: 65 536 units = 8 per wave).
#ifndef HM_VAL3_WG_PER_CU
#define HM_VAL3_WG_PER_CU (U % 3 != 0 ? 12 : 8)
#endif
    int wg_per_cu = HM_VAL3_WG_PER_CU;
    if (HM_TUNE_NF != 0 && k.variant >= 10000) wg_per_cu = k.variant / 10000;
    unsigned grid = MAP == 1 ? static_cast<unsigned>(units < cu_count() * 8 ? units : cu_count() * 8) : stream_grid(units, 4, wg_per_cu);   // 8 workgroups of 4 waves per CU
    if (U % 3 != 0 && grid >= 3) grid -= grid % 3;          // the unit index must advance by a multiple of 3 per iteration (see the kernel)
    if (grid == 0) grid = 1;
    if (describe_only(CH == 1 ? (FLAT ? "merge_u8_val3<N=%d,U=%d,PF=%d,MAP=%d,flat=1,C=1>" : "merge_u8_val3<N=%d,U=%d,PF=%d,MAP=%d,C=1>")
                              : (FLAT ? "merge_u8_val3<N=%d,U=%d,PF=%d,MAP=%d,flat=1>" : "merge_u8_val3<N=%d,U=%d,PF=%d,MAP=%d>"), NF, U, PF, MAP, QUAD)) return HM_OK;
    hipLaunchKernelGGL((merge_u8_val3<NF, U, PF, MAP, FLAT, CH, OUT, QUAD>), dim3(grid), dim3(256), 0, st, k);
    return launch_status();
}
// the 7UPM variant matrix of a tuning build (N == HM_TUNE_NF, float64 outputs)
template <int NF>
static int launch_val3_tune(const MergeK& k, hipStream_t st) {
    Val3Cfg c;
    if (!val3_variant(k.variant, NF, c)) return HM_EINVAL;
    switch (c.u * 100 + c.pf * 10 + c.map) {
        case 300: return launch_val3_cfg<NF, 3, 0, 0>(k, st);
        case 301: return launch_val3_cfg<NF, 3, 0, 1>(k, st);
        case 310: return launch_val3_cfg<NF, 3, 1, 0>(k, st);
        case 311: return launch_val3_cfg<NF, 3, 1, 1>(k, st);
        case 200: return launch_val3_cfg<NF, 2, 0, 0>(k, st);
        case 201: return launch_val3_cfg<NF, 2, 0, 1>(k, st);
        case 210: return launch_val3_cfg<NF, 2, 1, 0>(k, st);
        case 211: return launch_val3_cfg<NF, 2, 1, 1>(k, st);
        case 100: return launch_val3_cfg<NF, 1, 0, 0>(k, st);
        case 212: return launch_val3_cfg<NF, 2, 1, 2>(k, st);
        case 312: return launch_val3_cfg<NF, 3, 1, 2>(k, st);
        case 412: return launch_val3_cfg<NF, 4, 1, 2>(k, st);
        case 410: return launch_val3_cfg<NF, 4, 1, 0>(k, st);
        case 413: return launch_val3_cfg<NF, 4, 1, 3>(k, st);
        case 213: return launch_val3_cfg<NF, 2, 1, 3>(k, st);
        case 303: return launch_val3_cfg<NF, 3, 0, 3>(k, st);
        case 313: return launch_val3_cfg<NF, 3, 1, 3>(k, st);
        case 402: return launch_val3_cfg<NF, 4, 0, 2>(k, st);
        case 400: return launch_val3_cfg<NF, 4, 0, 0>(k, st);
        case 510: return launch_val3_cfg<NF, 5, 1, 0>(k, st);
        case 610: return launch_val3_cfg<NF, 6, 1, 0>(k, st);
        case 810: return launch_val3_cfg<NF, 8, 1, 0>(k, st);
        case 600: return launch_val3_cfg<NF, 6, 0, 0>(k, st);
        case 800: return launch_val3_cfg<NF, 8, 0, 0>(k, st);
        default:  return launch_val3_cfg<NF, 1, 1, 0>(k, st);
    }
}

template <int NF, int U, int TAB, bool PF>
static int launch_val_blk(const MergeK& k, const FastCfg& c, hipStream_t st) {
    if (c.block == 256) return launch_one<NF, U, TAB, false, PF, false, false, 256>(k, st);
    return launch_one<NF, U, TAB, false, PF, false, false, 1024>(k, st);
}

template <int NF, int U, bool PF>
static int launch_val_tab(const MergeK& k, const FastCfg& c, hipStream_t st) {
    switch (c.tab) {
        case TAB_PLAIN: return launch_val_blk<NF, U, TAB_PLAIN, PF>(k, c, st);
        case TAB_FUSED: return launch_val_blk<NF, U, TAB_FUSED, PF>(k, c, st);
#ifdef HM_PROBE
        default:        return launch_val_blk<NF, U, TAB_NONE, PF>(k, c, st);
#else
        default:        return HM_EINVAL;
#endif
    }
}

template <int NF, bool STD, int U, int TAB, int OUT = OUT_F64>
static int launch_extras(const MergeK& k, hipStream_t st) {
    const bool flat = k.has_flat != 0, sumw = k.out_sum_w != nullptr;
    if (flat && sumw) return launch_one<NF, U, TAB, STD, true, true, true, 256, 3, OUT>(k, st);
    if (flat) return launch_one<NF, U, TAB, STD, true, true, false, 256, 3, OUT>(k, st);
    return launch_one<NF, U, TAB, STD, true, false, true, 256, 3, OUT>(k, st);
}

#if HM_TUNE_NF != 0
#include "../../tools/hm_merge_priv_launch.inc"
#endif

// hm_merge_std_table on colour stacks of up to kLutTemplatedN frames with float64 outputs (hm_merge_host.h), with or without a flat field
template <int NF>
static int launch_fast_lut(const MergeK& k, hipStream_t st) {
    constexpr int U = HM_LUT_U;
    constexpr int OUT = OUT_F64;
    const bool flat = k.has_flat != 0;
    if (describe_only("merge_u8_fast_std<N=%d,U=%d,flat=%d,sum_w=%d>", NF, U, flat, 0)) return HM_OK;
    const int lds = kStdTabBytes + (flat ? 16 * 256 : 0);
    const unsigned grid = stream_grid(k.n_elems / (U * static_cast<int>(kSub)), 4, 8);
    if (flat) hipLaunchKernelGGL((merge_u8_fast_std_lut<NF, U, true, OUT>), dim3(grid), dim3(256), lds, st, k);
    else hipLaunchKernelGGL((merge_u8_fast_std_lut<NF, U, false, OUT>), dim3(grid), dim3(256), lds, st, k);
    return launch_status();
}

// merge_u8_val3 in its production configuration. Float32 outputs: the four-elements-per-lane map (16-byte stores) where the
// configuration has whole 256-element spans (val3_quad_cfg) and the call's alignment allows dword loads (quad_ok), else the pair map
template <int NF, bool FLAT, int CH, int OUT>
static int launch_val3_default(const MergeK& k, bool quad_ok, hipStream_t st) {
    constexpr Val3Cfg c = FLAT ? val3_flat_default(NF) : val3_default(NF);
    if constexpr (OUT == OUT_F32 && val3_quad_cfg(c)) {
        if (quad_ok) return launch_val3_cfg<NF, c.u, c.pf, c.map, FLAT, CH, OUT, true>(k, st);
    }
    return launch_val3_cfg<NF, c.u, c.pf, c.map, FLAT, CH, OUT, false>(k, st);
}

// Everything behind one frame count and output type. The variant matrix of a tuning build and the per-DN std table's kernel are float64
// instantiations only (a tuning build refuses variant > 0 for float32 calls, and float32 table calls stream at run-time N).
template <int NF, int OUT>
int launch_fast_nf(const MergeK& k, const FastCfg& c, bool with_std, bool allow_quad, hipStream_t st) {
    constexpr bool TUNE = OUT == OUT_F64 && NF == HM_TUNE_NF;
    if constexpr (OUT == OUT_F64 && NF <= kLutTemplatedN) {
        if (k.std_lut) return launch_fast_lut<NF>(k, st);
    }
    const bool extras = k.has_flat || k.out_sum_w;
    if (with_std) {
        if (use_fast_std_mono(k, true, false)) {
            if (k.has_flat) return launch_one<NF, kUStd, TAB_PLAIN, true, true, true, false, 256, 1, OUT>(k, st);
            return launch_one<NF, kUStd, TAB_PLAIN, true, true, false, false, 256, 1, OUT>(k, st);
        }
        if (extras) return launch_extras<NF, true, kUStd, TAB_PLAIN, OUT>(k, st);
        if constexpr (TUNE) {
            if (c.prefetch) {
                if (c.u == 1) return launch_one<NF, 1, TAB_PLAIN, true, true, false, false, 256>(k, st);
                if (c.u == 2) return launch_one<NF, 2, TAB_PLAIN, true, true, false, false, 256>(k, st);
                return launch_one<NF, 4, TAB_PLAIN, true, true, false, false, 256>(k, st);
            }
            if (c.u == 1) return launch_one<NF, 1, TAB_PLAIN, true, false, false, false, 256>(k, st);
            if (c.u == 2) return launch_one<NF, 2, TAB_PLAIN, true, false, false, false, 256>(k, st);
            return launch_one<NF, 4, TAB_PLAIN, true, false, false, false, 256>(k, st);
        }
        return launch_one<NF, kUStd, TAB_PLAIN, true, true, false, false, 256, 3, OUT>(k, st);
    }
    bool quad_ok = false;
    if constexpr (OUT == OUT_F32) {
        quad_ok = allow_quad && aligned(k.out_val, 16) && (!k.has_flat || !k.flat_u8 || aligned(k.flat_u8, 4));
        for (int i = 0; i < NF && quad_ok; ++i) quad_ok = aligned(static_cast<const uint8_t*>(k.frame[i]) + k.in_off, 4);
    }
    if (use_val3_mono(k, false, false)) {
        if (k.has_flat) return launch_val3_default<NF, true, 1, OUT>(k, quad_ok, st);
        return launch_val3_default<NF, false, 1, OUT>(k, quad_ok, st);
    }
    if (use_val3_flat(k, false)) return launch_val3_default<NF, true, 3, OUT>(k, quad_ok, st);
    if (extras) return launch_extras<NF, false, kUVal, TAB_FUSED, OUT>(k, st);
    if constexpr (TUNE) {
#if HM_TUNE_NF != 0
        int pu = 0;
        if (priv_variant(k.variant, NF, pu)) return launch_priv<NF>(k, st);
#endif
        if (use_val3(k.variant, NF, false, false)) return launch_val3_tune<NF>(k, st);
        if (c.prefetch) {
            if (c.u == 2) return launch_val_tab<NF, 2, true>(k, c, st);
            if (c.u == 4) return launch_val_tab<NF, 4, true>(k, c, st);
            return launch_val_tab<NF, 8, true>(k, c, st);
        }
        if (c.u == 2) return launch_val_tab<NF, 2, false>(k, c, st);
        if (c.u == 4) return launch_val_tab<NF, 4, false>(k, c, st);
        return launch_val_tab<NF, 8, false>(k, c, st);
    } else {
        if (use_val3(k.variant, NF, false, false)) return launch_val3_default<NF, false, 3, OUT>(k, quad_ok, st);
        return launch_one<NF, kUVal, TAB_FUSED, false, true, false, false, 256, 3, OUT>(k, st);      // variant > 0
    }
}

// hm_merge_std_f32 on colour stacks of the frame counts of kSd32Templated(), without a sum-of-weights output: merge_u8_fast_std reading
// float32 std frames, with the scheduling of the float64-std instantiation it stands beside (hm_merge_nf_sd32.hip instantiates these)
template <int NF, int OUT>
int launch_fast_nf_sd32(const MergeK& k, hipStream_t st) {
    if (k.has_flat) return launch_one<NF, kUStd, TAB_PLAIN, true, true, true, false, 256, 3, OUT, float>(k, st);
    return launch_one<NF, kUStd, TAB_PLAIN, true, true, false, false, 256, 3, OUT, float>(k, st);
}

// one line per frame count in a hm_merge_nf_*.hip unit
#define HM_INSTANTIATE_NF(n, OUT) template int launch_fast_nf<n, OUT>(HM_NF_ARGS);
#define HM_INSTANTIATE_NF_SD32(n, OUT) template int launch_fast_nf_sd32<n, OUT>(const MergeK&, hipStream_t);

}  // namespace hm
