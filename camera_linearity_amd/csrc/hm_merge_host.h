// hm_merge_host.h - host side shared by the fused merge's units (private to the hm_merge*.hip units; the file map is in hm_merge.hip):
// the describe context, the tuning-build environment knobs, the launch geometry the dispatcher and the launchers must agree on, and the
// family launchers the dispatcher calls. Every launcher is a function template that its own unit instantiates explicitly; the
// `extern template` declarations at the end keep every other unit - the dispatcher's first of all - from instantiating one, and with it
// the kernels behind it (a frame count no unit instantiates fails the link: -Wl,-z,defs).
#pragma once
#include "hm_merge_dev.h"
#include <cstdio>
#include <cstdlib>
#include <string>

#ifndef HM_TUNE_NF
#define HM_TUNE_NF 0      /* build with -DHM_TUNE_NF=7 to get the variant matrix for N = 7 */
#endif

namespace hm {

// hm_merge_describe(): the dispatch runs with this pointer set and every launch site records its kernel's name
// instead of launching - so the description cannot drift from what hm_merge really dispatches to.
struct DescribeCtx {
    std::string names;
    bool f32 = false;     // the call being described has out_kind = HM_OUT_F32
    bool lut = false;     // the call being described takes its stds from the per-DN table (hm_merge_std_table)
    bool sd32 = false;    // the call being described reads float32 std frames (hm_merge_std_f32)
};
extern thread_local DescribeCtx* g_describe;          // hm_merge.hip: set by merge_describe(), read by describe_only()
// quad: the kernel being named stores four float32 elements per lane (merge_u8_val3's QUAD map)
bool describe_only(const char* fmt, int a = 0, int b = 0, int c = 0, int d = 0, bool quad = false);

// experiment knobs of the tools/ A/B scripts, read from the environment in TUNING BUILDS only (-DHM_TUNE_NF=<N> or -DHM_TUNE_ENV): the shipped
// library never calls getenv. 0 = not set; values are clamped to [lo, hi] (a bmax above 64 or a per-CU count of 0 must not reach a launch).
inline int tune_env(const char* name, int lo, int hi) {
#if HM_TUNE_NF != 0 || defined(HM_TUNE_ENV)
    const char* v = getenv(name);
    const int e = v ? atoi(v) : 0;
    if (e == 0) return 0;
    return e < lo ? lo : (e > hi ? hi : e);
#else
    (void)name; (void)lo; (void)hi;
    return 0;
#endif
}

constexpr int kTemplatedN = 20;                    // frame counts with their own instantiation of the templated kernels (see hm_merge's dispatch)

// Variant encoding (args->variant; values other than 0 are meaningful in tuning builds only):
//   variant = 1000 * TAB + 100 * PREFETCH + 10 * U + BLOCK_CODE     U in {2,4,8}; BLOCK_CODE: 0 -> 256 threads, 1 -> 1024
struct FastCfg { int tab, u, prefetch, block; };

// Units per group (U sub-units of 128 elements) of the production configurations:
constexpr int kUVal = 2;     // val-only: 256 contiguous bytes per frame per wave iteration, next group prefetched
                             // (132-136 us on every box seen; without prefetch 135-146 us depending on the box)
constexpr int kUStd = 1;     // with std: one 128-element sub-unit per iteration + prefetch (tune: 684 us vs 753 at U = 2, no prefetch)

inline FastCfg default_cfg(bool with_std) {
    if (with_std) return FastCfg{TAB_PLAIN, kUStd, 1, 256};
    return FastCfg{TAB_FUSED, kUVal, 1, 256};     // tools/tune_merge.py, tools/mergelab.hip, profiles/
}

#ifndef HM_VAL3_FLAT_U
#define HM_VAL3_FLAT_U 2     // sub-units per iteration of merge_u8_val3's flat-field instantiation (N <= 8): 152 us at 134 VGPRs against 156 us at 176 VGPRs with U = 4
#endif

#ifndef HM_LUT_U
#define HM_LUT_U 1           // sub-units per group of merge_u8_fast_std_lut (with its other two knobs in hm_merge_nf.h)
#endif

// the val-only, no-extras configuration runs merge_u8_val3 unless a variant asks for the older merge_u8_fast (A/B runs).
// variant 7UPM (tuning builds, N == HM_TUNE_NF only) selects merge_u8_val3<NF, U, PF, MAP>; 0 = the production choice.
struct Val3Cfg { int u, pf, map; };
// Production choice per frame count (A/B on one box, tools/ab_val3.py): up to 8 frames <U=2, PF=1> - 64 VGPRs, 125.5 us on config 2
// against 130.0 us for merge_u8_fast and 133-135 us for the in-place refill (profiles/r02_ab_val3_matrix2.json); above that the second
// register set costs occupancy (N = 15: 137 VGPRs) and the in-place refill with U = 3 wins (82 VGPRs; config-4 tile 105.0 us against
// 109.3 us for both <2, 1> and merge_u8_fast, profiles/r02_ab_val3_n15.json).
// Late round 2: U = 4 with the second register set (115 VGPRs at N = 7) beats U = 2 by 1.3-1.9 us on three boxes, fast and slow (same-process A/B,
// shared outputs: 130.2 / 130.3 / 136.4 against 132.1 / 132.0 / 137.9 us, profiles/r02h_ab_val3_u4.log) - 512 contiguous bytes per frame and 4 KB of
// output per wave iteration; U = 5, 6, 8 and issuing a unit's stores together at its end (MAP = 2) are slower.
// Round 3: software-pipelined gathers (MAP = 3: the ds_read_b128 of the next bundle of 4 frames in flight under the current bundle's add / fma
// chain, two sets of gathered values, 158 VGPRs = 3 waves/SIMD at N = 7) are 2.0 us faster than MAP = 0 in three same-process A/B runs with
// shared output buffers on two boxes (129.25 / 126.1 / 128.5 against 131.3 / 128.1 / 130.2 us, profiles/r03_ab_pipe_n7_box*.json) and make no
// difference for N = 15 (<3, 0, 3> 105.1 against 105.2 us at 133 instead of 82 VGPRs; profiles/r03_ab_pipe_n15_box1.json), which keeps MAP = 0.
// N = 8 takes three sub-units per wave instead of four: 73.0 against 77.9 us on 2048 x 4096 x 3 stacks (0.689 against 0.646; a sweep of every
// frame count with a dip in tools/bench_n.py - 6, 8, 10, 16 - late in round 4: profiles/r04x_sweep8.log, r04x_sweep6_10_16.log; the others
// are within 3 % of their best variant as they stand).
// N = 9 and N = 10 take two sub-units (with / without the second register set): 78.8 against 81.2 us and 84.8 against 89.4 us
// (profiles/r04x_sweep9_14.log); 11-14 are within 1 % of their best variant with the shape of N = 15.
constexpr Val3Cfg val3_default(int n_frames) {
    return n_frames <= 7 ? Val3Cfg{4, 1, 3} : n_frames == 8 ? Val3Cfg{3, 1, 3} : n_frames == 9 ? Val3Cfg{2, 1, 0} : n_frames == 10 ? Val3Cfg{2, 0, 0}
                                                                                                                               : Val3Cfg{3, 0, 0};
}
inline bool val3_variant(int variant, int n_frames, Val3Cfg& c) {
    c = val3_default(n_frames);
    if (variant == 0) return true;
    variant %= 10000;                                     // (tuning builds: W * 10000 + 7UPM also sets the workgroups per CU, launch_val3_cfg)
    if (variant < 7000 || variant >= 8000 || n_frames != HM_TUNE_NF) return false;
    c.u = (variant / 100) % 10; c.pf = (variant / 10) % 10; c.map = variant % 10;
    return c.u >= 1 && c.u <= 8 && c.pf <= 1 && c.map <= 3;
}

// 8UMB: merge_u8_priv<N, U, MODE M, BLOCK = 256 | 768 | 1024 for B = 0 | 1 | 2> (tuning builds, N == HM_TUNE_NF; tools/hm_merge_priv*.inc)
inline bool priv_variant(int variant, int n_frames, int& u) {
    if (variant < 8000 || variant >= 9000 || n_frames != HM_TUNE_NF || HM_TUNE_NF == 0) return false;
    u = (variant / 100) % 10;
    const int m = (variant / 10) % 10, bcode = variant % 10;
    return (u == 2 || u == 4) && m <= 1 && bcode <= 2;
}

inline bool use_val3(int variant, int n_frames, bool with_std, bool extras) {
    Val3Cfg c;
    return !with_std && !extras && val3_variant(variant, n_frames, c);
}
// val-only WITH a uint8 flat field (no sum-of-weights output, library default variant): merge_u8_val3's FLAT instantiation
constexpr Val3Cfg val3_flat_default(int n_frames) { return n_frames <= 8 ? Val3Cfg{HM_VAL3_FLAT_U, 1, 3} : Val3Cfg{2, 1, 0}; }
// monochrome stacks (C == 1), val-only, at most a uint8 flat field, library default variant: merge_u8_val3's CH = 1 instantiations
inline bool use_val3_mono(const MergeK& k, bool with_std, bool f64in) {
    return !f64in && k.C == 1 && !with_std && !k.out_sum_w && k.variant == 0 && k.n_frames <= 16 && (!k.has_flat || k.flat_u8);
}
// ... and with std (with or without a flat field): merge_u8_fast_std's CH = 1 instantiations
inline bool use_fast_std_mono(const MergeK& k, bool with_std, bool f64in) {
    return !f64in && k.C == 1 && with_std && !k.out_sum_w && k.variant == 0 && k.n_frames <= 16;
}
inline bool use_val3_flat(const MergeK& k, bool with_std) {
    return !with_std && k.has_flat && k.flat_u8 && !k.out_sum_w && k.variant == 0 && k.n_frames <= 16;
}
inline int val3_unit_elems(const Val3Cfg& c) { return c.u * (c.map == 1 ? 4 : 1) * static_cast<int>(kSub); }

// hm_merge_std_table on colour stacks of up to kLutTemplatedN frames with float64 outputs, with or without a flat field:
// merge_u8_fast_std_lut. The rarer shapes (sum-of-weights output, C != 3, more frames, float32 outputs) take merge_u8_loop_std's table
// instantiations - build time.
constexpr int kLutTemplatedN = 16;

inline bool use_fast_lut(const MergeK& k, bool f64in) {
    return k.std_lut && !f64in && k.C == 3 && k.n_frames <= kLutTemplatedN && !k.out_sum_w && k.variant == 0;
}

// float32 outputs: what launch_fast_nf() chooses in a build without the tuning matrix, with OUT_F32 stores (a tuning build refuses
// variant > 0 for float32 calls). Instantiated for the frame counts of kF32Templated() only; the others stream through the run-time-N kernels.
constexpr bool kF32Templated(int n_frames) { return n_frames == 7 || n_frames == 15; }
// merge_u8_val3 with float32 outputs: the four-elements-per-lane map (16-byte stores) where the configuration has whole 256-element spans
// and the call's alignment allows dword loads, else the pair map (8-byte stores)
constexpr bool val3_quad_cfg(Val3Cfg c) { return c.pf == 1 && c.u % 2 == 0 && (c.map == 0 || c.map == 3); }
constexpr int kVariantF32Pairs = 32;     // args->variant of a float32 call: the library default with the pair map forced (A/B of the store shape, tools/bench_merge_f32.py)

// hm_merge_std_f32 (float32 std frames): compile-time-N kernels for colour stacks of these frame counts (BASELINE configs 3 and 4), with or
// without a flat field, both output types; every other uint8 shape (other N, C != 3, a sum-of-weights output) streams through
// merge_u8_loop_std at run-time N - build time. float64 frames with float32 stds run in merge_generic (merge_f64_std reads float64 stds).
constexpr bool kSd32Templated(int n_frames) { return n_frames == 7 || n_frames == 15; }
inline bool use_fast_sd32(const MergeK& k, bool sd32, bool f64in) {
    return sd32 && !f64in && k.C == 3 && kSd32Templated(k.n_frames) && !k.out_sum_w && k.variant == 0;
}

// ------------------------------------------------------------------------------------------------
// family launchers (k.n_elems whole groups of the family's unit size, or any count for the generic and hot-pixel kernels)
// ------------------------------------------------------------------------------------------------
// hm_merge_nf.h, instantiated by hm_merge_nf_*.hip: the compile-time-N kernels. allow_quad: float32 calls may take merge_u8_val3's QUAD map.
template <int NF, int OUT> int launch_fast_nf(const MergeK& k, const FastCfg& c, bool with_std, bool allow_quad, hipStream_t st);
// ... and merge_u8_fast_std reading float32 std frames (use_fast_sd32), instantiated by hm_merge_nf_sd32.hip
template <int NF, int OUT> int launch_fast_nf_sd32(const MergeK& k, hipStream_t st);
// SD: element type of the std frames - double, or float for hm_merge_std_f32 (std calls without the per-DN table only), instantiated by
// units of their own (hm_merge_loop_sd32.hip, hm_merge_hot_sd32.hip)
// hm_merge_loop.h / hm_merge_f64.hip: run-time N, uint8 / float64 frames
template <int OUT, typename SD = double> int launch_loop(const MergeK& k, bool with_std, hipStream_t st);
template <int OUT> int launch_f64(const MergeK& k, bool with_std, hipStream_t st);
// hm_merge_hot.h: one element per thread, and the hot-pixel pass without / with the queue workspace
template <int OUT, typename SD = double> int launch_generic(const MergeK& k, bool f64in, bool with_std, hipStream_t st);
template <int OUT, typename SD = double> int launch_fixup(const MergeK& k, bool f64in, bool with_std, hipStream_t st);
template <int OUT, typename SD = double> int launch_hot_queue(const MergeK& k, bool f64in, bool with_std, uint32_t* ws, size_t ws_bytes, hipStream_t st);

#define HM_NF_ARGS const MergeK&, const FastCfg&, bool, bool, hipStream_t
#define HM_EXTERN_NF(n) extern template int launch_fast_nf<n, OUT_F64>(HM_NF_ARGS);
HM_EXTERN_NF(1) HM_EXTERN_NF(2) HM_EXTERN_NF(3) HM_EXTERN_NF(4) HM_EXTERN_NF(5) HM_EXTERN_NF(6) HM_EXTERN_NF(7) HM_EXTERN_NF(8)
HM_EXTERN_NF(9) HM_EXTERN_NF(10) HM_EXTERN_NF(11) HM_EXTERN_NF(12) HM_EXTERN_NF(13) HM_EXTERN_NF(14) HM_EXTERN_NF(15) HM_EXTERN_NF(16)
HM_EXTERN_NF(17) HM_EXTERN_NF(18) HM_EXTERN_NF(19) HM_EXTERN_NF(20)
static_assert(kTemplatedN == 20, "one HM_EXTERN_NF per templated frame count");
#undef HM_EXTERN_NF
extern template int launch_fast_nf<7, OUT_F32>(HM_NF_ARGS);
extern template int launch_fast_nf<15, OUT_F32>(HM_NF_ARGS);
static_assert(kF32Templated(7) && kF32Templated(15) && !kF32Templated(8), "one declaration per float32-templated frame count");
#define HM_EXTERN_SD32(n) \
    extern template int launch_fast_nf_sd32<n, OUT_F64>(const MergeK&, hipStream_t); \
    extern template int launch_fast_nf_sd32<n, OUT_F32>(const MergeK&, hipStream_t);
HM_EXTERN_SD32(7) HM_EXTERN_SD32(15)
static_assert(kSd32Templated(7) && kSd32Templated(15) && !kSd32Templated(8), "one declaration per float32-std-templated frame count");
#undef HM_EXTERN_SD32
#define HM_EXTERN_OUT(OUT) \
    extern template int launch_f64<OUT>(const MergeK&, bool, hipStream_t);
HM_EXTERN_OUT(OUT_F64)
HM_EXTERN_OUT(OUT_F32)
#undef HM_EXTERN_OUT
#define HM_EXTERN_OUT_SD(OUT, SD) \
    extern template int launch_loop<OUT, SD>(const MergeK&, bool, hipStream_t); \
    extern template int launch_generic<OUT, SD>(const MergeK&, bool, bool, hipStream_t); \
    extern template int launch_fixup<OUT, SD>(const MergeK&, bool, bool, hipStream_t); \
    extern template int launch_hot_queue<OUT, SD>(const MergeK&, bool, bool, uint32_t*, size_t, hipStream_t);
HM_EXTERN_OUT_SD(OUT_F64, double)
HM_EXTERN_OUT_SD(OUT_F32, double)
HM_EXTERN_OUT_SD(OUT_F64, float)
HM_EXTERN_OUT_SD(OUT_F32, float)
#undef HM_EXTERN_OUT_SD

}  // namespace hm
