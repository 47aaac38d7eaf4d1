// hm_merge_dev.h - what more than one kernel family of the fused merge uses on the device (private to the hm_merge*.hip units; the file
// map is in hm_merge.hip): the kernel arguments, the output stores, the per-element reference arithmetic every kernel reproduces, the
// hot-pixel queue's layout, and the LDS tables, loads and stores of the streaming kernels.
#pragma once
#include "hm_common.h"
#include <type_traits>

namespace hm {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// kernel arguments (passed by value in the kernarg segment; all loads from it are scalar)
// ------------------------------------------------------------------------------------------------
struct MergeK {
    const void*    frame[HM_MAX_FRAMES];   // uint8 or float64 frames, at image row buf_row0
    const double*  sd[HM_MAX_FRAMES];      // float64 std frames (or null); in a hm_merge_std_f32 call float32 frames, read through sd_as<float>()
    const uint8_t* dark[HM_MAX_FRAMES];    // per-frame dark DN map (or null)
    double  inv_t[HM_MAX_FRAMES];          // 1 / exposure
    int32_t dark_min[HM_MAX_FRAMES];       // hot iff dark >= dark_min
    const double* icrf;
    const double* icrf_diff;
    const double* w_lut;
    const double* dw_lut;
    const uint8_t* flat_u8;                // at image row row0
    const double*  flat_f64;
    const double*  flat_std;
    double ff_mean[HM_MAX_CHANNELS];
    double ff_std_mean[HM_MAX_CHANNELS];
    double* out_val;                       // at image row row0
    double* out_std;
    double* out_sum_w;
    int64_t n_elems;                       // elements this launch covers (starting at elem0)
    int64_t elem0;                         // first element, relative to row0 (tail launches)
    int64_t in_off;                        // (row0 - buf_row0) * W * C: offset of row0 inside the input buffers
    int64_t H, W, row0, buf_row0, buf_rows;
    int32_t n_frames, C, median_k, has_flat;
    int32_t inv_t_inrange;                 // every 1/exposure in [2^-300, 2^300] (host check; see div_inrange)
    int32_t variant;
    uint32_t* hot_reset;                   // the hot-pixel queue's four counter words, zeroed by the streaming kernel that runs before the scan
    const double* std_lut;                 // hm_merge_std_table: (256, C) per-DN std table read by the LUT instantiations instead of sd[] (else null)
    // std frame i with the element type of the instantiation (template parameter SD: double, or float for hm_merge_std_f32; the struct
    // itself carries no flag for it - the dispatcher picks the SD = float launchers - and keeps its layout)
    template <typename SD>
    __host__ __device__ __forceinline__ const SD* sd_as(int i) const { return reinterpret_cast<const SD*>(sd[i]); }
};

// The queue's counters must be zero when merge_scan_hot starts. A hipMemsetAsync costs two fill kernels (~10 us per call, 1 % of
// config 3); the streaming kernel that precedes the scan in stream order does it in passing instead (one wave-uniform test per workgroup).
__device__ __forceinline__ void reset_hot_counters(const MergeK& a) {
    if (a.hot_reset && blockIdx.x == 0 && threadIdx.x < 4) a.hot_reset[threadIdx.x] = 0u;
}

// Output element type (template parameter OUT). MergeK keeps out_val / out_std typed double*: with OUT_F32 they address float arrays.
enum { OUT_F64 = HM_OUT_F64, OUT_F32 = HM_OUT_F32 };
template <int OUT>
__device__ __forceinline__ void store_out(double* base, int64_t e, double x) {         // element e of an output array
    if constexpr (OUT == OUT_F64) base[e] = x;
    else reinterpret_cast<float*>(base)[e] = static_cast<float>(x);
}
template <int OUT>
__device__ __forceinline__ double* out_at(double* base, int64_t e) {                   // address of element e (scalar bases of the streaming kernels)
    if constexpr (OUT == OUT_F64) return base + e;
    else return reinterpret_cast<double*>(reinterpret_cast<float*>(base) + e);
}

__device__ __forceinline__ void elem_to_pixel(const MergeK& a, int64_t e, int64_t& row, int64_t& col, int& c) {
    const int64_t wc = a.W * a.C;
    row = a.row0 + e / wc;
    const int64_t rem = e % wc;
    col = rem / a.C;
    c = static_cast<int>(rem % a.C);
}

__device__ __forceinline__ void flat_field_apply(const MergeK& a, int64_t e, int c, bool with_std,
                                                 double& val, double& sd) {
    const double F = a.flat_u8 ? static_cast<double>(a.flat_u8[e]) / 255.0 : a.flat_f64[e];
    flat_field_math(F, with_std ? 1.0 / (F * F) : 1.0, with_std ? a.flat_std[e] : 0.0, a.ff_mean[c], a.ff_std_mean[c], with_std, val, sd);
}

// index linearize forms from a frame value (measurand.py:503): the DN itself, or lut_index() of the float64 value
__device__ __forceinline__ uint32_t lut_index_of(uint8_t v) { return v; }
__device__ __forceinline__ uint32_t lut_index_of(double v) { return lut_index(v); }

// std of element `i` of frame `f` through the per-DN table (hm_merge_std_table): what linearize(frame, icrf = std_table).val holds there.
// Handed to the k x k medians as their element accessor: a hot frame's std is the median of the MAPPED neighbourhood (the reference
// filters the std image on its own, measurand.py:553-555), which differs from std_table[median DN] for a table that is not monotone.
template <typename T>
struct StdLutAt {
    const T* f; const double* lut; int C, c;
    __device__ __forceinline__ double operator()(int64_t i) const { return lut[lut_index_of(f[i]) * C + c]; }
};

// std of element `i` of a std frame of element type SD, widened to float64 (exact for float: hm_merge_std_f32). The k x k medians take it
// as their element accessor: widening is monotone, so the median of the widened neighbourhood is the widened median.
template <typename SD>
struct StdAt {
    const SD* s;
    __device__ __forceinline__ double operator()(int64_t i) const { return static_cast<double>(s[i]); }
};

// Hot-element queue in the caller's workspace (hm_merge_args.hot_workspace), uint32 words:
//   ws[0] = number of queued elements, ws[1] = overflow flag (the queue was too small: merge_patch_hot goes over the whole tile),
//   ws[2] = number of pieces the scan wrote (its workgroups x rounds), ws[3] unused;
//   ws[4 .. 4 + 2 T)  piece table, T = hot_piece_slots(n_elems): {queue offset, count} of piece p - a piece is what one scan workgroup
//                     queued in one round, 65 536 consecutive elements of the image, and p counts them in IMAGE order; the pieces land in
//                     the queue in the order of their atomics, the table lets the patch kernel walk them in image order;
//   ws[4 + 2 T ...]   element indices relative to row0 (uint32: the queue path requires fewer than 2^32 elements per call).
constexpr int kHotQueueHeader = 4;       // uint32 words before the piece table (16 bytes)
constexpr int kHotPiecesLds = 2048;      // pieces the patch kernel can order in LDS (134 M elements per call); beyond that it walks the queue as it lies
__host__ __device__ inline uint32_t hot_piece_slots(int64_t n_elems) { return static_cast<uint32_t>(n_elems / 65536 + 1 + 1024); }

// ------------------------------------------------------------------------------------------------
// One output element: the reference arithmetic (exposure_series.py:340-394) in the operation sequence
// shared by every kernel of the merge, so a result does not depend on which kernel (or tiling) produced
// it: S = sum_i w_i in frame order; 1/S and 1/S**2 formed once; the numerator of :388 accumulated with
// fma and divided by S at the end; variance terms of :389 accumulated with fma.
// HOT = HOT_NONE: plain per-thread evaluation, dark maps ignored (streaming kernels).
// HOT = HOT_WAVE: `e` is wave-uniform, every lane evaluates the same element and hot frames take their value
//                 from wave_median(); `store` selects the one lane that writes.
// HOT = HOT_LANE: every lane evaluates its OWN element and takes the medians of its hot frames itself
//                 (lane_median(); the queue-driven patch kernel).
// Tables: t_w/t_dw [256], t_g/t_d [256*C] in LDS.
// ------------------------------------------------------------------------------------------------
enum { HOT_NONE = 0, HOT_WAVE = 1, HOT_LANE = 2 };
// LUT (hm_merge_std_table): the frames' stds come from a.std_lut (global memory: these are the cold paths) instead of a.sd[].
// SD (hm_merge_std_f32): element type of the std frames; a float std is widened once, on its way into a register.
template <bool F64IN, bool STD, int HOT, int OUT = OUT_F64, bool LUT = false, typename SD = double>
__device__ __forceinline__ void merge_one_element(const MergeK& a, const double* t_w, const double* t_dw,
                                                  const double* t_g, const double* t_d, int64_t e, bool store) {
    const int C = a.C, N = a.n_frames;
    const int64_t ei = a.in_off + e;
    const int c = static_cast<int>(e % C);
    int64_t row = 0, col = 0; int cc = 0;
    if (HOT != HOT_NONE) elem_to_pixel(a, e, row, col, cc);
    auto is_hot = [&](int i) -> bool { return HOT != HOT_NONE && a.dark[i] && static_cast<int>(a.dark[i][ei]) >= a.dark_min[i]; };
    auto median_of = [&](auto* f) {
        if constexpr (HOT == HOT_WAVE) return wave_median(f, a.H, a.W, C, a.buf_row0, row, col, cc, a.median_k);
        else return lane_median(f, a.H, a.W, C, a.buf_row0, row, col, cc, a.median_k);
    };
    auto value_f64 = [&](int i, bool hot) -> double {
        const double* f = static_cast<const double*>(a.frame[i]);
        if (HOT != HOT_NONE && hot) return median_of(f);
        return f[ei];
    };
    auto value_u8 = [&](int i, bool hot) -> uint32_t {
        const uint8_t* f = static_cast<const uint8_t*>(a.frame[i]);
        if (HOT != HOT_NONE && hot) return median_of(f);
        return f[ei];
    };
    // ---- pass 1: S = sum_i w_i (exposure_series.py:340) ----
    double S = 0.0;
    for (int i = 0; i < N; ++i) {
        const bool hot = is_hot(i);
        double w;
        if (F64IN) {
            const double dv = value_f64(i, hot) - 0.5;
            w = gauss_weight(dv);                                 // measurand.py:615
        } else {
            w = t_w[value_u8(i, hot)];
        }
        S = (i == 0) ? w : S + w;
    }
    if (a.out_sum_w && store) a.out_sum_w[e] = S;
    if (!a.out_val) return;
    const double invS = 1.0 / S;
    const double invS2 = 1.0 / (S * S);                                 // 1 / S**2, exposure_series.py:343
    // ---- pass 2: exposure_series.py:382-389 ----
    double acc = 0.0, var = 0.0;
    for (int i = 0; i < N; ++i) {
        const bool hot = is_hot(i);
        double w, dw;
        uint32_t idx;
        if (F64IN) {
            const double v = value_f64(i, hot);
            const double dv = v - 0.5;
            w = gauss_weight(dv);
            dw = gauss_dweight(dv, w);                                  // measurand.py:616
            idx = lut_index(v);                                         // measurand.py:503
        } else {
            idx = value_u8(i, hot);
            w = t_w[idx];
            dw = STD ? t_dw[idx] : 0.0;
        }
        const double g = t_g[idx * C + c];
        const double it = a.inv_t[i];
        const double wg = w * g;
        acc = (i == 0) ? wg * it : fma(wg, it, acc);                    // :388 numerator
        if (STD) {
            double s;
            if constexpr (LUT) {
                using T = std::conditional_t<F64IN, double, uint8_t>;
                const StdLutAt<T> at{static_cast<const T*>(a.frame[i]), a.std_lut, C, c};
                if (HOT != HOT_NONE && hot) {
                    if constexpr (HOT == HOT_WAVE) s = wave_median_of(at, a.H, a.W, C, a.buf_row0, row, col, cc, a.median_k);
                    else s = lane_median_of<double>(at, a.H, a.W, C, a.buf_row0, row, col, cc, a.median_k);
                } else s = a.std_lut[idx * C + c];
            } else if constexpr (std::is_same_v<SD, double>) {
                if (HOT != HOT_NONE && hot) s = median_of(a.sd[i]);
                else s = a.sd[i][ei];
            } else {
                const StdAt<SD> at{a.template sd_as<SD>(i)};
                if (HOT != HOT_NONE && hot) {
                    if constexpr (HOT == HOT_WAVE) s = wave_median_of(at, a.H, a.W, C, a.buf_row0, row, col, cc, a.median_k);
                    else s = lane_median_of<double>(at, a.H, a.W, C, a.buf_row0, row, col, cc, a.median_k);
                } else s = at(ei);
            }
            const double dg = t_d[idx * C + c] * s;                     // measurand.py:512
            const double term = merge_var_term(w, dw, g, dg, invS, invS2, it);    // :389
            var = (i == 0) ? term * term : fma(term, term, var);
        }
    }
    double val = acc / S;
    double sd = STD ? sqrt(var) : 0.0;                                  // :394
    if (a.has_flat) flat_field_apply(a, e, c, STD, val, sd);
    if (store) {
        store_out<OUT>(a.out_val, e, val);
        if (STD) store_out<OUT>(a.out_std, e, sd);
    }
}

template <bool F64IN, bool STD>
__device__ __forceinline__ void fill_plain_tables(const MergeK& a, double* t_w, double* t_dw, double* t_g, double* t_d) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        t_w[i] = (!F64IN) ? a.w_lut[i] : 0.0;
        t_dw[i] = (!F64IN && STD) ? a.dw_lut[i] : 0.0;
    }
    for (int i = threadIdx.x; i < 256 * a.C; i += blockDim.x) {
        t_g[i] = a.icrf[i];
        t_d[i] = STD ? a.icrf_diff[i] : 0.0;
    }
}

// LDS table layouts of the val-only kernel:
//   TAB_PLAIN   w[256] | wg[256*3]  (8-byte entries, two ds_read_b64 per (element, frame))        8 KB
//   TAB_FUSED   {w, wg}[256*3] as 16-byte entries, one ds_read_b128 per (element, frame)          12 KB
//   TAB_NONE    (tuning probe only, wrong results) no gather at all: the HBM ceiling of the access pattern
// Replicating the tables across banks was measured and dropped (docs/DESIGN_history_r01_r02.md 4.4): only a full private copy
// per lane of an LDS lane group removes the ~2.4-way conflicts random DNs cause, and that needs 64 KB per
// 256-entry float64 table, i.e. one workgroup per CU, which loses more latency hiding than it gains.
// The std kernel uses {w,dw}[256] and {g,d}[768] as 16-byte entries (16 KB).
enum { TAB_PLAIN = 0, TAB_FUSED = 1, TAB_NONE = 5 };

template <int TAB> struct TabInfo;
template <> struct TabInfo<TAB_PLAIN> { static constexpr int bytes = 8 * 256 * 4; };
template <> struct TabInfo<TAB_FUSED> { static constexpr int bytes = 16 * 768; };
template <> struct TabInfo<TAB_NONE>  { static constexpr int bytes = 16; };
constexpr int kStdTabBytes = 16 * 256 + 16 * 768;

__device__ __forceinline__ uint32_t ld_u16(const uint8_t* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p));
}
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
}
// the same load through an explicit global-address-space pointer: after an `asm volatile("+s")` pin the compiler no longer
// knows that a kernarg pointer is global and would fall back to flat_load (which also counts against lgkmcnt)
// 16-byte nontemporal load at (scalar base) + (32-bit byte offset in a VGPR) through an explicit global-address-space pointer:
// after an `asm volatile("+s")` pin hipcc no longer knows that a kernarg pointer is global and emits flat_load, which
// counts against lgkmcnt as well as vmcnt and so serialises with the LDS gathers around it.
typedef const __attribute__((address_space(1))) f64x2* global_f64x2_ptr;
typedef const __attribute__((address_space(1))) char* global_char_ptr;
__device__ __forceinline__ f64x2 ld_f64x2_global(const double* scalar_base, uint32_t byte_off) {
    global_char_ptr g = (global_char_ptr)(scalar_base);
    return __builtin_nontemporal_load((global_f64x2_ptr)(g + byte_off));
}

// Buffer addressing for the frame bytes: the frame pointer sits in a 4-SGPR resource descriptor, the group's byte offset
// in one SGPR shared by all frames (soffset), the lane's offset in one VGPR and the sub-unit in the immediate - a load
// costs no address arithmetic at all (global_load needs a 64-bit VGPR address or a 64-bit scalar base per frame and group).
// Raw buffer, stride 0, num_records = 2^32 - 1 bytes: offsets are below 2^32 because the fast kernels require E < 2^32.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t frame_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0xffffffff, 0x00020000);
}
constexpr int kAuxNT = 2;                                             // cache-policy bits of the raw-buffer builtins on gfx94x/gfx950: nt
__device__ __forceinline__ uint16_t ld_u16_buf(__amdgpu_buffer_rsrc_t r, uint32_t lane_off, uint32_t group_off) {
    return __builtin_amdgcn_raw_buffer_load_b16(r, static_cast<int>(lane_off), static_cast<int>(group_off), kAuxNT);
}
// The lane's two stds of a 128-element sub-unit of a std frame (SD = double: the 16-byte load above; SD = float, hm_merge_std_f32: one
// 8-byte load, half the bytes and half the registers per frame) at (scalar base) + lane16 (float: lane16 / 2). sd_pair_x / _y widen.
typedef const __attribute__((address_space(1))) f32x2* global_f32x2_ptr;
template <typename SD> struct SdPair { typedef f64x2 type; };
template <> struct SdPair<float> { typedef f32x2 type; };
template <typename SD>
__device__ __forceinline__ typename SdPair<SD>::type ld_sd_pair_global(const SD* scalar_base, uint32_t lane16) {
    if constexpr (std::is_same_v<SD, double>) return ld_f64x2_global(scalar_base, lane16);
    else {
        global_char_ptr g = (global_char_ptr)(scalar_base);
        return __builtin_nontemporal_load((global_f32x2_ptr)(g + (lane16 >> 1)));
    }
}
// the same load through a generic pointer (merge_u8_loop_std)
template <typename SD>
__device__ __forceinline__ typename SdPair<SD>::type ld_sd_pair(const SD* base, uint32_t lane16) {
    if constexpr (std::is_same_v<SD, double>)
        return __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(reinterpret_cast<const char*>(base) + lane16));
    else return __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(reinterpret_cast<const char*>(base) + (lane16 >> 1)));
}
// store two float64 at (scalar base) + (32-bit byte offset in a VGPR)
__device__ __forceinline__ void store2(double* base, uint32_t byte_off, double x, double y) {
    f64x2 v; v.x = x; v.y = y;
    __builtin_nontemporal_store(v, reinterpret_cast<f64x2*>(reinterpret_cast<char*>(base) + byte_off));
}

// the lane's two elements of a 128-element sub-unit that starts at `base`: 16 bytes per lane as float64 (one contiguous 1 KB
// global_store_dwordx4 per wave), 8 bytes per lane as float32 (one contiguous 512-byte global_store_dwordx2: four whole 128-byte lines)
template <int OUT>
__device__ __forceinline__ void store_pair(double* base, uint32_t lane16, double x, double y) {
    if constexpr (OUT == OUT_F64) store2(base, lane16, x, y);
    else {
        f32x2 v; v.x = static_cast<float>(x); v.y = static_cast<float>(y);
        __builtin_nontemporal_store(v, reinterpret_cast<f32x2*>(reinterpret_cast<char*>(base) + (lane16 >> 1)));
    }
}

// four consecutive float32 elements of one lane (merge_u8_val3's QUAD map): one contiguous 1 KB global_store_dwordx4 per wave
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_quad_f32(double* base, uint32_t lane16, float x0, float x1, float x2, float x3) {
    f32x4 v; v.x = x0; v.y = x1; v.z = x2; v.w = x3;
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(reinterpret_cast<char*>(base) + lane16));
}

template <int TAB>
__device__ __forceinline__ void fill_val_tables(char* lds, const MergeK& a) {
    constexpr int C = 3;
    if constexpr (TAB == TAB_NONE) return;
    for (int q = threadIdx.x; q < 256 * C; q += blockDim.x) {
        const int dn = q / C;
        const double w = a.w_lut[dn];
        const double wg = w * a.icrf[q];             // (w * g), exposure_series.py:388
        if constexpr (TAB == TAB_PLAIN) {
            double* t = reinterpret_cast<double*>(lds);
            if (q % C == 0) t[dn] = w;
            t[256 + q] = wg;
        } else {
            reinterpret_cast<double2*>(lds)[q] = double2{w, wg};
        }
    }
}

template <int TAB>
__device__ __forceinline__ uint32_t chan_off(uint32_t c) {
    if constexpr (TAB == TAB_PLAIN) return 2048u + c * 8u;
    if constexpr (TAB == TAB_FUSED) return c * 16u;
    return c;
}
template <int TAB>
__device__ __forceinline__ void gather_val(const char* lds, uint32_t dn, uint32_t coff, double& w, double& wg) {
    if constexpr (TAB == TAB_NONE) {
        w = static_cast<double>(dn + 1u); wg = static_cast<double>(dn + coff);
    } else if constexpr (TAB == TAB_PLAIN) {
        w = *reinterpret_cast<const double*>(lds + dn * 8u);
        wg = *reinterpret_cast<const double*>(lds + dn * 24u + coff);
    } else {
        const double2 t = *reinterpret_cast<const double2*>(lds + dn * 48u + coff);
        w = t.x; wg = t.y;
    }
}

// keeps an accumulator chain where the source puts it (hipcc otherwise sinks the second element's chain
// below the first element's epilogue and keeps every gathered value live until then)
#define HM_PIN(x) asm volatile("" : "+v"(x))

constexpr uint32_t kSub = 128;     // elements per sub-unit (64 lanes x 2)

}  // namespace hm
