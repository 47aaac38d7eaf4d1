// hm_host.cpp - HOST build of the C ABI of include/hdrmerge.h (libhdrmerge_host.so).
//
// The reference's factory returns a NumPy (host) Measurand for use_cupy=False (modules/measurand_factory.py:10-14,
// modules/measurand.py:684-714), which is also BASELINE.json's configs[0] ("NumPy Measurand CPU merge, plumbing, no GPU").
// This file backs that slot: the same entry points as libhdrmerge.so with HOST pointers - `stream` is ignored, calls are
// synchronous, workspaces may be NULL - written from scratch in plain C++ (g++ -O2 -fopenmp, no HIP, no NumPy, nothing from
// oracle/). It is selected EXPLICITLY (Measurand(use_cupy=False) / HostMeasurand); the HIP backend never falls back to it.
//
// Arithmetic: the operation sequence of the device kernels, element by element. The element formulas are the ../csrc/hm_*_math.h headers
// included below, the text the device kernels compile too; where the builds differ on purpose the header's top comment says so.
// Statistics use the reference's own two-pass form.
// Since round 4 also the upstream producers (hm_welford_*, hm_linearity_energy: SURVEY.md 8f-2/3). Not here:
// the two TIFF strip decoders hm_tiff_lzw_decode / hm_tiff_packbits_decode (host code already, in libhdrmerge.so) and the hm_debug_* probes.
// hm_tiff_decode_strips, the device path of those files, has its host-pointer twin at the end of this file, followed by the twins of
// hm_tiff_decode_strips_wide (2-, 4- and 8-byte samples) and of hm_tiff_encode_strips / hm_tiff_encode_strips_wide, through which tiff_io.imwrite writes LZW strips.
//
// The argument rules of most entries are a check_* of the ../csrc/hm_*_rules.h headers included below, the copies the device build compiles
// too; where this build differs the check is called with hm_rules::HOST, and the header's top comment lists the difference.
#include "hdrmerge.h"
#include "../csrc/hm_merge_math.h"
#include "../csrc/hm_ops_math.h"
#include "../csrc/hm_stats_math.h"
#include "../csrc/hm_producer_math.h"
#include "../csrc/hm_merge_rules.h"
#include "../csrc/hm_calibration_rules.h"
#include "../csrc/hm_de_args.h"
#include "../csrc/hm_frame_rules.h"
#include "../csrc/hm_ops_rules.h"
#include "../csrc/hm_pairs_rules.h"
#include "../csrc/hm_producer_rules.h"
#include "../csrc/hm_tiff_rules.h"
#include "../csrc/hm_tiff_lzw_body.h"
#include "../csrc/hm_tiff_lzw_enc_body.h"
#include "../csrc/hm_tiff_wide_body.h"
#include "../csrc/hm_tiff_wide_enc_body.h"

#ifdef _OPENMP
#include <omp.h>
#endif
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

namespace {

constexpr double kNaN = std::numeric_limits<double>::quiet_NaN();
constexpr double kInf = std::numeric_limits<double>::infinity();
using hm_rules::aligned8, hm_rules::dense_elems;
using namespace hm;                                   // the element formulas of the hm_*_math.h headers

// k x k median of one channel around one pixel; buf holds image rows [buf_row0, ...)
template <typename T>
inline T median_at(const T* buf, int64_t H, int64_t W, int C, int64_t buf_row0, int64_t row, int64_t col, int c, int k) {
    T v[49];
    const int r = k / 2;
    int n = 0;
    for (int dy = -r; dy <= r; ++dy) {
        const int64_t yy = reflect_index(row + dy, H) - buf_row0;
        for (int dx = -r; dx <= r; ++dx) {
            const int64_t xx = reflect_index(col + dx, W);
            v[n++] = buf[(yy * W + xx) * C + c];
        }
    }
    std::nth_element(v, v + n / 2, v + n);
    return v[n / 2];
}

// the same median over the neighbourhood mapped through `at(value)` (hm_merge_std_table: the per-DN std of every neighbour; the reference
// filters the std image on its own, measurand.py:553-555)
template <typename T, typename At>
inline double median_mapped_at(const T* buf, At at, int64_t H, int64_t W, int C, int64_t buf_row0, int64_t row, int64_t col, int c, int k) {
    double v[49];
    const int r = k / 2;
    int n = 0;
    for (int dy = -r; dy <= r; ++dy) {
        const int64_t yy = reflect_index(row + dy, H) - buf_row0;
        for (int dx = -r; dx <= r; ++dx) {
            const int64_t xx = reflect_index(col + dx, W);
            v[n++] = at(buf[(yy * W + xx) * C + c]);
        }
    }
    std::nth_element(v, v + n / 2, v + n);
    return v[n / 2];
}

// flat-field epilogue of merge element e of channel c: flat_field_apply of hm_merge_dev.h (the uint16 entries have no uint8 flat)
inline void flat_apply(const hm_merge_args* g, int64_t e, int c, bool with_std, double& val, double& sd) {
    const double F = g->flat_u8 ? static_cast<double>(g->flat_u8[e]) / 255.0 : g->flat_f64[e];
    flat_field_math(F, with_std ? 1.0 / (F * F) : 1.0, with_std ? g->flat_std[e] : 0.0, g->ff_mean[c], g->ff_std_mean[c], with_std, val, sd);
}

// the two operands' offsets of element e of a checked broadcast (hm_rules::check_bcast)
inline void bcast_offsets(int ndim, const int64_t* shape, const int64_t* st1, const int64_t* st2, int64_t e, int64_t& o1, int64_t& o2) {
    o1 = 0; o2 = 0;
    for (int d = ndim - 1; d >= 0; --d) {
        const int64_t i = e % shape[d];
        e /= shape[d];
        o1 += i * st1[d];
        o2 += i * st2[d];
    }
}

// compute_dimension_statistics of ONE reduction line given by an accessor (measurand.py:337-347): NaN-ignoring, weights 1/std
template <typename Get>
inline void line_statistics(int64_t n, bool weighted, Get get, double& mean, double& sd, double& err) {
    if (!weighted) {
        double s = 0.0; int64_t cnt = 0;
        for (int64_t k = 0; k < n; ++k) { double v, u; get(k, v, u); if (v == v) { s += v; ++cnt; } }
        mean = cnt ? s / static_cast<double>(cnt) : kNaN;                          // nanmean
        double q = 0.0;
        for (int64_t k = 0; k < n; ++k) { double v, u; get(k, v, u); if (v == v) { const double d = v - mean; q += d * d; } }
        sd = cnt ? std::sqrt(q / static_cast<double>(cnt)) : kNaN;                 // nanstd
        err = kNaN;
        return;
    }
    double sw = 0.0, svw = 0.0, ss = 0.0; int64_t cs = 0;
    for (int64_t k = 0; k < n; ++k) {
        double v, u; get(k, v, u);
        const double w = 1.0 / u;                                                  // :342
        if (w == w) sw += w;                                                       // nansum(weights)
        const double vw = v * w;
        if (vw == vw) svw += vw;                                                   // nansum(values * weights)
        if (u == u) { ss += u; ++cs; }
    }
    mean = svw / sw;                                                               // :344
    double q = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        double v, u; get(k, v, u);
        const double w = 1.0 / u;
        const double d = v - mean;
        const double t = w * (d * d);                                              // :345
        if (t == t) q += t;
    }
    sd = std::sqrt(q / sw);
    err = cs ? ss / static_cast<double>(cs) : kNaN;                                // nanmean(stds)
}

}  // namespace

extern "C" {

int hm_version(void) { return HM_ABI_VERSION; }

const char* hm_strerror(int code) {
    switch (code) {
        case HM_OK: return "ok";
        case HM_EINVAL: return "invalid argument";
        case HM_EUNSUPPORTED: return "unsupported configuration (host build: channels > HM_MAX_CHANNELS, or a device-only entry point)";
        case HM_EALIGN: return "float64 buffer is not 8-byte aligned";
        case HM_ELAUNCH: return "launch failed";
        case HM_ENODEVICE: return "no usable gfx950 device";
        case HM_ESHAPE: return "inconsistent geometry (tile outside image or median halo missing)";
        default: return "unknown hdrmerge error";
    }
}

int hm_device_info(int* n_devices, int* cu_count, int* lds_bytes, char* arch, int arch_len) {
    if (n_devices) *n_devices = 0;
    if (cu_count) *cu_count = 0;
    if (lds_bytes) *lds_bytes = 0;
    if (arch && arch_len > 0) { std::strncpy(arch, "host", static_cast<size_t>(arch_len) - 1); arch[arch_len - 1] = 0; }
    return HM_OK;
}

// ---- rows 1, 3, 4 -------------------------------------------------------------------------------------------------
int hm_gaussian_weight_f64(const double* v, double* w, double* dw, int64_t n, void*) {
    if (n < 0 || (n > 0 && !v)) return HM_EINVAL;
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        const double dv = v[e] - 0.5;
        const double y = gauss_weight(dv);
        if (w) w[e] = y;
        if (dw) dw[e] = gauss_dweight(dv, y);                                     // measurand.py:616
    }
    return HM_OK;
}

int hm_gaussian_weight_u8(const uint8_t* dn, const double* w_lut, const double* dw_lut, double* w, double* dw, int64_t n, void*) {
    if (n < 0 || (n > 0 && (!dn || (w && !w_lut) || (dw && !dw_lut)))) return HM_EINVAL;
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        if (w) w[e] = w_lut[dn[e]];
        if (dw) dw[e] = dw_lut[dn[e]];
    }
    return HM_OK;
}

int hm_gaussian_weight_lut_host(double* w_lut, double* dw_lut) { return hm_rules::gaussian_weight_lut(8, w_lut, dw_lut); }
int hm_gaussian_weight_lut_bits_host(int bit_depth, double* w_lut, double* dw_lut) { return hm_rules::gaussian_weight_lut(bit_depth, w_lut, dw_lut); }

int hm_u8_to_unit_f64(const uint8_t* dn, double* out, int64_t n, void*) {
    if (n < 0 || (n > 0 && (!dn || !out))) return HM_EINVAL;
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) out[e] = static_cast<double>(dn[e]) / 255.0;   // image_set.py:223
    return HM_OK;
}

static int linearize_any(const uint8_t* dn, const double* v, const double* std_, const double* icrf, const double* icrf_diff,
                         double* out_val, double* out_std, uint8_t* out_idx, int64_t n, int C, int lut_stride) {
    if (const int rc = hm_rules::check_linearize(v != nullptr, dn ? static_cast<const void*>(dn) : v, std_, icrf, out_val, out_std, n, C, lut_stride,
                                                 hm_rules::HOST); rc != HM_OK) return rc;
    const bool use_std = std_ && icrf_diff && out_std;                            // measurand.py:498-500
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        const uint32_t k = dn ? dn[e] : lut_index(v[e]);                          // :505 / :503
        const int64_t at = lut_stride == 1 ? k : static_cast<int64_t>(k) * C + (e % C);
        out_val[e] = icrf[at];
        if (use_std) out_std[e] = icrf_diff[at] * std_[e];                        // :512
        if (out_idx) out_idx[e] = static_cast<uint8_t>(k);
    }
    return HM_OK;
}
int hm_linearize_u8(const uint8_t* dn, const double* std_, const double* icrf, const double* icrf_diff, double* out_val, double* out_std,
                    int64_t n, int C, int lut_stride, void*) {
    return linearize_any(dn, nullptr, std_, icrf, icrf_diff, out_val, out_std, nullptr, n, C, lut_stride);
}
int hm_linearize_f64(const double* v, const double* std_, const double* icrf, const double* icrf_diff, double* out_val, double* out_std,
                     uint8_t* out_idx, int64_t n, int C, int lut_stride, void*) {
    return linearize_any(nullptr, v, std_, icrf, icrf_diff, out_val, out_std, out_idx, n, C, lut_stride);
}
// uint16 DNs: idx = dn & (2^bit_depth - 1), tables of 2^bit_depth rows
int hm_linearize_u16(const uint16_t* dn, const double* std_, const double* icrf, const double* icrf_diff, double* out_val, double* out_std,
                     uint16_t* out_idx, int64_t n, int C, int lut_stride, int bit_depth, void*) {
    if (const int rc = hm_rules::check_linearize_u16(dn, std_, icrf, out_val, out_std, out_idx, n, C, lut_stride, bit_depth); rc != HM_OK) return rc;
    const bool use_std = std_ && icrf_diff && out_std;                            // measurand.py:498-500
    const uint32_t mask = (1u << bit_depth) - 1u;
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        const uint32_t k = static_cast<uint32_t>(dn[e]) & mask;
        const int64_t at = lut_stride == 1 ? k : static_cast<int64_t>(k) * C + (e % C);
        out_val[e] = icrf[at];
        if (use_std) out_std[e] = icrf_diff[at] * std_[e];                        // :512
        if (out_idx) out_idx[e] = static_cast<uint16_t>(k);
    }
    return HM_OK;
}

// ---- rows 5-9: the merge ------------------------------------------------------------------------------------------
size_t hm_merge_hot_workspace_bytes(int64_t) { return 16; }
size_t hm_merge_hot_workspace_min_bytes(int64_t) { return 16; }
size_t hm_merge_frames_workspace_bytes(int, int64_t, int) { return 0; }           // any number of frames in one pass on the host

// The argument rules of the three entries and the byte count: ../csrc/hm_merge_rules.h, the copy the device build compiles too. This build
// adds no refusal of its own.
using hm_rules::MergeCall;
using hm_rules::MergeEntry;

int64_t hm_merge_algorithmic_bytes(const hm_merge_args* g) { return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_MERGE); }
int64_t hm_merge_std_table_algorithmic_bytes(const hm_merge_args* g) { return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_STD_TABLE); }
int64_t hm_merge_std_f32_algorithmic_bytes(const hm_merge_args* g) { return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_STD_F32); }

// extra: the entry's own pointer (hm_merge_rules.h). The std entries return for NULL args before anything else is read - or written.
static int merge_describe(const hm_merge_args* g, MergeEntry entry, const void* extra, char* buf, int buf_len) {
    if (!buf || buf_len < 1 || (!g && entry != hm_rules::ENTRY_MERGE)) return HM_EINVAL;
    MergeCall call;
    const int rc = hm_rules::check_merge_call(g, entry, extra, call);
    if (rc == HM_OK && !call.empty)
        std::snprintf(buf, static_cast<size_t>(buf_len), "merge_host<f64in=%d,std=%d,hot=%d%s%s>(N=%d)", call.f64in, call.with_std, call.hot,
                      call.std_src == hm_rules::STD_TABLE ? ",std=lut" : call.std_src == hm_rules::STD_F32 ? ",std=f32" : "",
                      call.f32out ? ",out=f32" : "", call.a.n_frames);
    else buf[0] = 0;
    return rc;
}
int hm_merge_describe(const hm_merge_args* g, char* buf, int buf_len) { return merge_describe(g, hm_rules::ENTRY_MERGE, nullptr, buf, buf_len); }
int hm_merge_std_table_describe(const hm_merge_args* g, const double* std_table, char* buf, int buf_len) {
    return merge_describe(g, hm_rules::ENTRY_STD_TABLE, std_table, buf, buf_len);
}
int hm_merge_std_f32_describe(const hm_merge_args* g, const float* const* stds_f32, char* buf, int buf_len) {
    return merge_describe(g, hm_rules::ENTRY_STD_F32, stds_f32, buf, buf_len);
}

// exposure_series.py:340-394 per output element, the operation sequence of merge_one_element() (hm_merge_dev.h): S in frame order;
// 1/S and 1/S**2 once; numerator and variance accumulated with fma in frame order; acc / S last; flat field last.
}  // extern "C" (templates below)

// One instantiation per (float64 frames, dark maps, std) combination: the per-element loop carries no run-time mode tests, and the row / column
// of an element are only worked out where a median needs them. Same operations in the same order in every instantiation.
// std_table (hm_merge_std_table; g->stds is NULL then): a frame's std is std_table[idx * C + c], idx the index linearize forms from the
// frame's own value; for a hot frame the median of the neighbourhood's mapped values.
// sd32 (hm_merge_std_f32): g->stds addresses float32 frames; each std is widened (exactly) as it is read, a hot frame's after its median
// (widening is monotone: the same element either way).
template <bool F64IN, bool HOT, bool STD>
static void merge_elements(const hm_merge_args* g, const double* inv_t, int k, const double* std_table, bool sd32) {
    const int N = g->n_frames, C = g->channels;
    const auto std32 = [g](int i) { return reinterpret_cast<const float*>(g->stds[i]); };
    const bool flat = g->flat_u8 || g->flat_f64;
    const int64_t W = g->width, wc = W * C, E = g->rows * wc;
    const int64_t in_off = (g->row0 - g->buf_row0) * wc;
    std::vector<double> wg_store;
    if (!F64IN && !STD && g->out_val) {
        wg_store.resize(static_cast<size_t>(256) * C);
        for (int q = 0; q < 256 * C; ++q) wg_store[static_cast<size_t>(q)] = g->w_lut[q / C] * g->icrf[q];
    }
    const double* const wg_tab = wg_store.data();
    // out_kind: the float64 result rounded once (to nearest even) at the store - static_cast<float> - into 4-byte elements
    const bool f32out = g->out_kind == HM_OUT_F32;
    const auto put = [f32out](double* base, int64_t e, double x) {
        if (f32out) reinterpret_cast<float*>(base)[e] = static_cast<float>(x); else base[e] = x;
    };
#pragma omp parallel
    {
        std::vector<double> vv(static_cast<size_t>(N)), ss(static_cast<size_t>(N));
        std::vector<uint32_t> dd(static_cast<size_t>(N));
        double* const v = vv.data(); double* const sdv = ss.data(); uint32_t* const dn = dd.data();
        // this thread's contiguous range of elements; the channel index runs along with e (a 64-bit remainder per element cost as much as
        // the rest of a val-only element)
        int64_t lo = 0, hi = E;
#ifdef _OPENMP
        {
            const int64_t nt = omp_get_num_threads(), tid = omp_get_thread_num();
            lo = E * tid / nt; hi = E * (tid + 1) / nt;
        }
#endif
        if constexpr (!F64IN && !STD && !HOT) {
            // val-only on DNs without dark maps (BASELINE config 2's arithmetic): four elements at a time - four independent sum / fma chains
            // per frame instead of one (the chains are latency-bound: 7 dependent adds and 7 dependent fmas per element) - from the w g
            // table; the same operations per element in the same order as the one-element loop below, which takes the tail.
            if (wg_tab) {
                constexpr int B = 4;
                int cb[B];
                for (; lo + B <= hi; lo += B) {
                    const int64_t ei = in_off + lo;
                    for (int j = 0; j < B; ++j) cb[j] = static_cast<int>((lo + j) % C);
                    double S4[B], a4[B];
                    for (int i = 0; i < N; ++i) {
                        const uint8_t* p = g->frames_u8[i] + ei;
                        const double it = inv_t[i];
                        for (int j = 0; j < B; ++j) {
                            const uint32_t d = p[j];
                            const double w = g->w_lut[d], wg = wg_tab[d * C + cb[j]];
                            S4[j] = i == 0 ? w : S4[j] + w;                          // exposure_series.py:340
                            a4[j] = i == 0 ? wg * it : std::fma(wg, it, a4[j]);      // :388 numerator
                        }
                    }
                    for (int j = 0; j < B; ++j) {
                        const int64_t e = lo + j;
                        if (g->out_sum_w) g->out_sum_w[e] = S4[j];
                        double val = a4[j] / S4[j], none = 0.0;
                        if (flat) flat_apply(g, e, cb[j], false, val, none);
                        put(g->out_val, e, val);
                    }
                }
            }
        }
        int c = static_cast<int>(lo % C) - 1;
        for (int64_t e = lo; e < hi; ++e) {
            const int64_t ei = in_off + e;
            c = c + 1 == C ? 0 : c + 1;
            // the (filtered) frame values of this element
            if constexpr (HOT) {
                const int64_t row = g->row0 + e / wc, col = (e % wc) / C;
                for (int i = 0; i < N; ++i) {
                    const bool h = g->darks_u8[i] && static_cast<int>(g->darks_u8[i][ei]) >= g->dark_min_dn[i];   // measurand.py:545
                    if constexpr (F64IN) v[i] = h ? median_at(g->frames_f64[i], g->height, W, C, g->buf_row0, row, col, c, k) : g->frames_f64[i][ei];
                    else dn[i] = h ? median_at(g->frames_u8[i], g->height, W, C, g->buf_row0, row, col, c, k) : g->frames_u8[i][ei];
                    if constexpr (STD) {
                        if (std_table) {
                            const auto at_u8 = [=](uint8_t x) { return std_table[static_cast<uint32_t>(x) * C + c]; };
                            const auto at_f64 = [=](double x) { return std_table[lut_index(x) * C + c]; };
                            if constexpr (F64IN) sdv[i] = h ? median_mapped_at(g->frames_f64[i], at_f64, g->height, W, C, g->buf_row0, row, col, c, k) : at_f64(g->frames_f64[i][ei]);
                            else sdv[i] = h ? median_mapped_at(g->frames_u8[i], at_u8, g->height, W, C, g->buf_row0, row, col, c, k) : at_u8(g->frames_u8[i][ei]);
                        } else if (sd32) sdv[i] = static_cast<double>(h ? median_at(std32(i), g->height, W, C, g->buf_row0, row, col, c, k) : std32(i)[ei]);
                        else sdv[i] = h ? median_at(g->stds[i], g->height, W, C, g->buf_row0, row, col, c, k) : g->stds[i][ei];
                    }
                }
            } else {
                for (int i = 0; i < N; ++i) {
                    if constexpr (F64IN) v[i] = g->frames_f64[i][ei]; else dn[i] = g->frames_u8[i][ei];
                    if constexpr (STD) {
                        if (!std_table) sdv[i] = sd32 ? static_cast<double>(std32(i)[ei]) : g->stds[i][ei];
                        else if constexpr (F64IN) sdv[i] = std_table[lut_index(v[i]) * C + c];
                        else sdv[i] = std_table[dn[i] * C + c];
                    }
                }
            }
            double S = 0.0;
            if (!F64IN && !STD && wg_tab) {
                // val-only on DNs: S and the numerator in ONE walk over the frames, the product w g from a table built once per call
                // (wg_tab[dn C + c] = w_lut[dn] * icrf[dn C + c]: the same product of the same operands, the same bits)
                double acc1 = 0.0;
                const double* tab = wg_tab + c;
                for (int i = 0; i < N; ++i) {
                    const uint32_t d = dn[i];
                    const double w = g->w_lut[d];
                    S = i == 0 ? w : S + w;                                          // exposure_series.py:340
                    acc1 = i == 0 ? tab[d * C] * inv_t[i] : std::fma(tab[d * C], inv_t[i], acc1);   // :388 numerator
                }
                if (g->out_sum_w) g->out_sum_w[e] = S;
                if (!g->out_val) continue;
                double val1 = acc1 / S;
                double none = 0.0;
                if (flat) flat_apply(g, e, c, false, val1, none);
                put(g->out_val, e, val1);
                continue;
            }
            for (int i = 0; i < N; ++i) {
                double w;
                if constexpr (F64IN) w = gauss_weight(v[i] - 0.5); else w = g->w_lut[dn[i]];
                S = i == 0 ? w : S + w;                                              // exposure_series.py:340
            }
            if (g->out_sum_w) g->out_sum_w[e] = S;
            if (!g->out_val) continue;
            const double invS = 1.0 / S, invS2 = 1.0 / (S * S);                     // :343
            double acc = 0.0, var = 0.0;
            for (int i = 0; i < N; ++i) {
                double w, dw = 0.0; uint32_t idx;
                if constexpr (F64IN) {
                    const double dv = v[i] - 0.5;
                    w = gauss_weight(dv);
                    dw = gauss_dweight(dv, w);
                    idx = lut_index(v[i]);
                } else {
                    idx = dn[i];
                    w = g->w_lut[idx];
                    if constexpr (STD) dw = g->dw_lut[idx];
                }
                const double gg = g->icrf[idx * C + c];
                const double it = inv_t[i];
                const double wg = w * gg;
                acc = i == 0 ? wg * it : std::fma(wg, it, acc);                     // :388 numerator
                if constexpr (STD) {
                    const double dg = g->icrf_diff[idx * C + c] * sdv[i];                                // measurand.py:512
                    const double term = merge_var_term(w, dw, gg, dg, invS, invS2, it);                  // :389
                    var = i == 0 ? term * term : std::fma(term, term, var);
                }
            }
            double val = acc / S;
            double sd = STD ? std::sqrt(var) : 0.0;                                 // :394
            if (flat) flat_apply(g, e, c, STD, val, sd);
            put(g->out_val, e, val);
            if constexpr (STD) put(g->out_std, e, sd);
        }
    }
}

// hm_merge_u16: uint16 DN frames, tables of 2^bit_depth rows read at idx = DN & mask. One pass over the elements with the operation
// sequence of merge_elements' general loop (no per-DN std table, float64 std frames, the float64 flat field).
// HOT (hm_merge_u16_darks, merge_u16_darks_host): darks[i] is frame i's uint16 dark map or NULL; where (dark & mask) >= dark_min_dn[i] the
// frame's masked DN is the k x k median of the masked DNs around it and its std the k x k median of the std neighbourhood, filtered inline
// into the element's idx_of[] / sd_of[] - then the same operations in the same order, so the bits of hm_merge_u16 on pre-filtered frames.
// Without HOT (hm_merge_u16) nothing is staged: idx_at / sd_at read the frames as that path always did.
// std_table (hm_merge_u16_std_table): frame i's std is std_table[idx_i C + c] instead of g->stds[i] (NULL there); a hot frame's is the k x k
// median of the mapped neighbourhood, median_j(std_table[idx_j C + c]) - what the median of a materialised std frame is.
template <bool STD, bool HOT = false>
static void merge_elements_u16(const hm_merge_args* g, const uint16_t* const* frames, uint32_t mask, const double* inv_t,
                               const uint16_t* const* darks = nullptr, const double* std_table = nullptr) {
    const int N = g->n_frames, C = g->channels;
    const bool flat = g->flat_f64 != nullptr;
    const int64_t wc = g->width * C, E = g->rows * wc;
    const int64_t in_off = (g->row0 - g->buf_row0) * wc;
    const bool f32out = g->out_kind == HM_OUT_F32;
    const auto put = [f32out](double* base, int64_t e, double x) {
        if (f32out) reinterpret_cast<float*>(base)[e] = static_cast<float>(x); else base[e] = x;
    };
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < E; ++e) {
        const int64_t ei = in_off + e;
        const int c = static_cast<int>(e % C);
        [[maybe_unused]] uint32_t idx_of[HOT ? HM_MAX_FRAMES : 1];
        [[maybe_unused]] double sd_of[HOT && STD ? HM_MAX_FRAMES : 1];
        if constexpr (HOT) {
            const int k = g->median_k;
            const auto masked = [mask](uint16_t x) { return static_cast<double>(x & mask); };      // exact, order-preserving
            for (int i = 0; i < N; ++i) {
                idx_of[i] = frames[i][ei] & mask;
                if constexpr (STD) sd_of[i] = std_table ? std_table[idx_of[i] * C + c] : g->stds[i][ei];
                if (darks[i] && static_cast<int>(darks[i][ei] & mask) >= g->dark_min_dn[i]) {
                    const int64_t row = g->row0 + e / wc, col = (e % wc) / C;
                    idx_of[i] = static_cast<uint32_t>(median_mapped_at(frames[i], masked, g->height, g->width, C, g->buf_row0, row, col, c, k));
                    if constexpr (STD) {
                        const auto tabled = [=](uint16_t x) { return std_table[(x & mask) * C + c]; };
                        sd_of[i] = std_table ? median_mapped_at(frames[i], tabled, g->height, g->width, C, g->buf_row0, row, col, c, k)
                                             : median_at(g->stds[i], g->height, g->width, C, g->buf_row0, row, col, c, k);
                    }
                }
            }
        }
        const auto idx_at = [&](int i) -> uint32_t { if constexpr (HOT) return idx_of[i]; else return frames[i][ei] & mask; };
        [[maybe_unused]] const auto sd_at = [&](int i) -> double {
            if constexpr (HOT) return sd_of[i];
            else return std_table ? std_table[(frames[i][ei] & mask) * C + c] : g->stds[i][ei];
        };
        double S = 0.0;
        for (int i = 0; i < N; ++i) {
            const double w = g->w_lut[idx_at(i)];
            S = i == 0 ? w : S + w;                                              // exposure_series.py:340
        }
        if (g->out_sum_w) g->out_sum_w[e] = S;
        if (!g->out_val) continue;
        const double invS = 1.0 / S, invS2 = 1.0 / (S * S);                     // :343
        double acc = 0.0, var = 0.0;
        for (int i = 0; i < N; ++i) {
            const uint32_t idx = idx_at(i);
            const double w = g->w_lut[idx];
            const double gg = g->icrf[idx * C + c];
            const double it = inv_t[i];
            const double wg = w * gg;
            acc = i == 0 ? wg * it : std::fma(wg, it, acc);                     // :388 numerator
            if constexpr (STD) {
                const double dw = g->dw_lut[idx];
                const double dg = g->icrf_diff[idx * C + c] * sd_at(i);                               // measurand.py:512
                const double term = merge_var_term(w, dw, gg, dg, invS, invS2, it);                  // :389
                var = i == 0 ? term * term : std::fma(term, term, var);
            }
        }
        double val = acc / S;
        double sd = STD ? std::sqrt(var) : 0.0;                                 // :394
        if (flat) flat_apply(g, e, c, STD, val, sd);
        put(g->out_val, e, val);
        if constexpr (STD) put(g->out_std, e, sd);
    }
}

// The uint16 entries, shaped like merge_run / merge_describe below: the rules of `entry` (ENTRY_U16 / ENTRY_U16_DARKS / ENTRY_U16_STD_TABLE),
// then the one loop. A hm_merge_u16_darks call whose maps are all NULL has call.hot = false: it runs, and answers, as hm_merge_u16.
static int merge_u16_run(MergeEntry entry, const hm_merge_args* g_in, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, int bit_depth,
                         const double* std_table = nullptr) {
    const hm_rules::U16Extra x{frames_u16, bit_depth, darks_u16, std_table};
    MergeCall call;
    const int rc = hm_rules::check_merge_call(g_in, entry, &x, call);
    if (rc != HM_OK || call.empty) return rc;
    const hm_merge_args* g = &call.a;
    std::vector<double> inv_t(static_cast<size_t>(g->n_frames));
    for (int i = 0; i < g->n_frames; ++i) inv_t[static_cast<size_t>(i)] = 1.0 / g->exposures[i];
    const uint32_t mask = (1u << call.bit_depth) - 1u;
    const bool with_std = call.with_std && g->out_val;
    if (call.hot) {                                                     // the hot-pixel filter inline in merge_elements_u16
        if (with_std) merge_elements_u16<true, true>(g, call.frames_u16, mask, inv_t.data(), call.darks_u16, call.std_table);
        else merge_elements_u16<false, true>(g, call.frames_u16, mask, inv_t.data(), call.darks_u16);
    } else if (with_std) merge_elements_u16<true>(g, call.frames_u16, mask, inv_t.data(), nullptr, call.std_table);
    else merge_elements_u16<false>(g, call.frames_u16, mask, inv_t.data());
    return HM_OK;
}

static int merge_u16_describe(MergeEntry entry, const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, int bit_depth,
                              char* buf, int buf_len, const double* std_table = nullptr) {
    if (!buf || buf_len < 1 || !g) return HM_EINVAL;
    const hm_rules::U16Extra x{frames_u16, bit_depth, darks_u16, std_table};
    MergeCall call;
    const int rc = hm_rules::check_merge_call(g, entry, &x, call);
    buf[0] = 0;
    if (rc != HM_OK || call.empty) return rc;
    char hot[24] = "";
    if (call.hot) std::snprintf(hot, sizeof hot, ",hot=%d", call.a.median_k);
    const bool with_std = call.with_std && call.a.out_val;
    std::snprintf(buf, static_cast<size_t>(buf_len), "merge_u16_host<tab=host,bits=%d,C=%d,std=%s%s%s>(N=%d)", call.bit_depth, call.a.channels,
                  with_std ? (call.std_table ? "lut" : "1") : "0", hot, call.f32out ? ",out=f32" : "", call.a.n_frames);
    return rc;
}

extern "C" {

int64_t hm_merge_u16_algorithmic_bytes(const hm_merge_args* g) { return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_U16); }
int64_t hm_merge_u16_darks_algorithmic_bytes(const hm_merge_args* g, const uint16_t* const* darks_u16) {
    return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_U16_DARKS, darks_u16);
}

int hm_merge_u16(const hm_merge_args* g, const uint16_t* const* frames_u16, int bit_depth, void*) {
    return merge_u16_run(hm_rules::ENTRY_U16, g, frames_u16, nullptr, bit_depth);
}
int hm_merge_u16_describe(const hm_merge_args* g, const uint16_t* const* frames_u16, int bit_depth, char* buf, int buf_len) {
    return merge_u16_describe(hm_rules::ENTRY_U16, g, frames_u16, nullptr, bit_depth, buf, buf_len);
}
int hm_merge_u16_darks(const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, int bit_depth, void*) {
    return merge_u16_run(hm_rules::ENTRY_U16_DARKS, g, frames_u16, darks_u16, bit_depth);
}
int hm_merge_u16_darks_describe(const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, int bit_depth,
                                char* buf, int buf_len) {
    return merge_u16_describe(hm_rules::ENTRY_U16_DARKS, g, frames_u16, darks_u16, bit_depth, buf, buf_len);
}

int64_t hm_merge_u16_std_table_algorithmic_bytes(const hm_merge_args* g, const uint16_t* const* darks_u16) {
    return hm_rules::merge_algorithmic_bytes(g, hm_rules::ENTRY_U16_STD_TABLE, darks_u16);
}
int hm_merge_u16_std_table(const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16, const double* std_table,
                           int bit_depth, void*) {
    return merge_u16_run(hm_rules::ENTRY_U16_STD_TABLE, g, frames_u16, darks_u16, bit_depth, std_table);
}
int hm_merge_u16_std_table_describe(const hm_merge_args* g, const uint16_t* const* frames_u16, const uint16_t* const* darks_u16,
                                    const double* std_table, int bit_depth, char* buf, int buf_len) {
    return merge_u16_describe(hm_rules::ENTRY_U16_STD_TABLE, g, frames_u16, darks_u16, bit_depth, buf, buf_len, std_table);
}

static int merge_run(const hm_merge_args* g_in, MergeEntry entry, const void* extra) {
    MergeCall call;
    const int rc = hm_rules::check_merge_call(g_in, entry, extra, call);
    if (rc != HM_OK || call.empty) return rc;
    const hm_merge_args* g = &call.a;
    const int N = g->n_frames;
    const double* const std_table = call.std_table;
    const bool sd32 = call.std_src == hm_rules::STD_F32, f64in = call.f64in, hot = call.hot;
    const bool with_std = call.with_std && g->out_val != nullptr;                 // (float64 std frames without out_val: no std is formed)
    std::vector<double> inv_t(static_cast<size_t>(N));
    for (int i = 0; i < N; ++i) inv_t[static_cast<size_t>(i)] = 1.0 / g->exposures[i];
    const int k = hot ? g->median_k : 3;
    const int mode = (f64in ? 4 : 0) | (hot ? 2 : 0) | (with_std ? 1 : 0);
    switch (mode) {
        case 0: merge_elements<false, false, false>(g, inv_t.data(), k, std_table, sd32); break;
        case 1: merge_elements<false, false, true>(g, inv_t.data(), k, std_table, sd32); break;
        case 2: merge_elements<false, true, false>(g, inv_t.data(), k, std_table, sd32); break;
        case 3: merge_elements<false, true, true>(g, inv_t.data(), k, std_table, sd32); break;
        case 4: merge_elements<true, false, false>(g, inv_t.data(), k, std_table, sd32); break;
        case 5: merge_elements<true, false, true>(g, inv_t.data(), k, std_table, sd32); break;
        case 6: merge_elements<true, true, false>(g, inv_t.data(), k, std_table, sd32); break;
        default: merge_elements<true, true, true>(g, inv_t.data(), k, std_table, sd32); break;
    }
    return HM_OK;
}

int hm_merge(const hm_merge_args* g_in, void*) { return merge_run(g_in, hm_rules::ENTRY_MERGE, nullptr); }
int hm_merge_std_table(const hm_merge_args* g_in, const double* std_table, void*) { return merge_run(g_in, hm_rules::ENTRY_STD_TABLE, std_table); }
int hm_merge_std_f32(const hm_merge_args* g_in, const float* const* stds_f32, void*) { return merge_run(g_in, hm_rules::ENTRY_STD_F32, stds_f32); }

}  // extern "C"

// ---- row 8 standalone ---------------------------------------------------------------------------------------------
template <typename T>
static int hot_filter(const T* x, const uint8_t* map_u8, const double* map_f64, int min_dn, double thr, int k, T* out,
                      int64_t H, int64_t W, int C) {
    if (H < 0 || W < 0 || C < 1) return HM_EINVAL;
    if (H * W * C == 0) return HM_OK;
    if (!x || !out || (!map_u8 == !map_f64) || k < 3 || k > 7 || (k % 2) == 0) return HM_EINVAL;
    const int64_t wc = W * C, n = H * wc;
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        const bool hot = map_u8 ? static_cast<int>(map_u8[e]) >= min_dn : map_f64[e] > thr;              // measurand.py:545
        out[e] = hot ? median_at(x, H, W, C, 0, e / wc, (e % wc) / C, static_cast<int>(e % C), k) : x[e];
    }
    return HM_OK;
}
extern "C" {
int hm_hot_pixel_filter_u8(const uint8_t* x, const uint8_t* map_u8, const double* map_f64, int min_dn, double thr, int median_k,
                           uint8_t* out, int64_t H, int64_t W, int C, void*) {
    return hot_filter(x, map_u8, map_f64, min_dn, thr, median_k, out, H, W, C);
}
int hm_hot_pixel_filter_f64(const double* x, const uint8_t* map_u8, const double* map_f64, int min_dn, double thr, int median_k,
                            double* out, int64_t H, int64_t W, int C, void*) {
    return hot_filter(x, map_u8, map_f64, min_dn, thr, median_k, out, H, W, C);
}

// ---- row 9 standalone ---------------------------------------------------------------------------------------------
size_t hm_roi_mean_workspace_bytes(void) { return 64; }
}  // extern "C"
template <typename T>
static int roi_mean(const T* img, int64_t H, int64_t W, int C, int64_t x0, int64_t x1, int64_t y0, int64_t y1, double* out, double scale) {
    if (!img || !out || C < 1 || C > HM_MAX_CHANNELS) return HM_EINVAL;
    if (x0 < 0 || y0 < 0 || x1 > H || y1 > W || x1 <= x0 || y1 <= y0) return HM_ESHAPE;
    double acc[HM_MAX_CHANNELS] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r = x0; r < x1; ++r)
        for (int64_t q = y0; q < y1; ++q)
            for (int c = 0; c < C; ++c) acc[c] += static_cast<double>(img[(r * W + q) * C + c]);
    const double cnt = static_cast<double>((x1 - x0) * (y1 - y0));
    for (int c = 0; c < C; ++c) out[c] = (acc[c] / scale) / cnt;                  // measurand.py:579 (uint8 images: DN / 255); k_roi_final's order
    return HM_OK;
}
extern "C" {
int hm_roi_mean_u8(const uint8_t* img, int64_t H, int64_t W, int C, int64_t x0, int64_t x1, int64_t y0, int64_t y1, double* out, void*, void*) {
    return roi_mean(img, H, W, C, x0, x1, y0, y1, out, 255.0);
}
int hm_roi_mean_f64(const double* img, int64_t H, int64_t W, int C, int64_t x0, int64_t x1, int64_t y0, int64_t y1, double* out, void*, void*) {
    return roi_mean(img, H, W, C, x0, x1, y0, y1, out, 1.0);
}
int hm_normalize_by_map(const double* val, const double* std_, const uint8_t* flat_u8, const double* flat_f64, const double* flat_std,
                        const double* ff_mean, const double* ff_std_mean, double* out_val, double* out_std, int64_t n, int C, void*) {
    if (n < 0 || C < 1 || C > HM_MAX_CHANNELS) return HM_EINVAL;
    if (n == 0) return HM_OK;
    if (!val || !out_val || !ff_mean || (!flat_u8 == !flat_f64)) return HM_EINVAL;
    if (out_std && (!std_ || !flat_std || !ff_std_mean)) return HM_EINVAL;
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        const int c = static_cast<int>(e % C);
        const double F = flat_u8 ? static_cast<double>(flat_u8[e]) / 255.0 : flat_f64[e];
        double v = val[e], s = out_std ? std_[e] : 0.0;
        flat_field_math(F, out_std ? 1.0 / (F * F) : 1.0, out_std ? flat_std[e] : 0.0, ff_mean[c], out_std ? ff_std_mean[c] : 0.0, out_std != nullptr, v, s);
        out_val[e] = v;
        if (out_std) out_std[e] = s;
    }
    return HM_OK;
}

// ---- row 10: operators (measurand.py:106-279) ----------------------------------------------------------------------
int hm_binary_op(int op, const double* x1, const double* s1, const double* x2, const double* s2, double* out_val, double* out_std,
                 int ndim, const int64_t* shape, const int64_t* strides1, const int64_t* strides2, void*) {
    int64_t n;
    if (const int rc = hm_rules::check_binary_op(op, x1, s1, x2, s2, out_val, out_std, ndim, shape, strides1, strides2, hm_rules::HOST, n);
        rc != HM_OK) return rc;
    const bool with_std = out_std != nullptr;
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        int64_t o1, o2;
        bcast_offsets(ndim, shape, strides1, strides2, e, o1, o2);
        const double a = x1[o1], c = x2[o2];
        const double sa = (with_std && s1) ? s1[o1] : 0.0, sc = (with_std && s2) ? s2[o2] : 0.0;       // missing std -> zeros (:121-124)
        double r, rs = 0.0;
        switch (op) {
            case HM_OP_ADD: binary_eval<HM_OP_ADD>(a, sa, c, sc, with_std, r, rs); break;
            case HM_OP_SUB: binary_eval<HM_OP_SUB>(a, sa, c, sc, with_std, r, rs); break;
            case HM_OP_MUL: binary_eval<HM_OP_MUL>(a, sa, c, sc, with_std, r, rs); break;
            case HM_OP_DIV: binary_eval<HM_OP_DIV>(a, sa, c, sc, with_std, r, rs); break;
            default: binary_eval<HM_OP_POW>(a, sa, c, sc, with_std, r, rs);
        }
        out_val[e] = r;
        if (with_std) out_std[e] = rs;
    }
    return HM_OK;
}

int hm_unary_op(int op, const double* x, const double* s, double* out_val, double* out_std, int64_t n, void*) {
    if (const int rc = hm_rules::check_unary_op(op, x, s, out_val, out_std, n, hm_rules::HOST); rc != HM_OK) return rc;
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        double r, rs = 0.0;
        unary_eval(op, x[e], out_std != nullptr, [&] { return s[e]; }, r, rs);
        out_val[e] = r;
        if (out_std) out_std[e] = rs;
    }
    return HM_OK;
}

int hm_pow_scalar(const double* x, const double* s, double exponent, double* out_val, double* out_std, int64_t n, void*) {
    if (const int rc = hm_rules::check_unary_op(HM_UOP_NEG, x, s, out_val, out_std, n, hm_rules::HOST); rc != HM_OK) return rc;
    const double p = exponent;
    const int kind = p == 2.0 ? POW_SQUARE : p == 0.5 ? POW_SQRT : p == 1.0 ? POW_ONE : POW_GENERAL;     // never POW_INT: hm_ops_math.h
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        const double v = x[e], sv = out_std ? s[e] : 0.0;
        double r, rs = 0.0;
        switch (kind) {
            case POW_SQUARE: pow_scalar_eval<POW_SQUARE>(v, sv, p, 0, out_std != nullptr, r, rs); break;
            case POW_SQRT: pow_scalar_eval<POW_SQRT>(v, sv, p, 0, out_std != nullptr, r, rs); break;
            case POW_ONE: pow_scalar_eval<POW_ONE>(v, sv, p, 0, out_std != nullptr, r, rs); break;
            default: pow_scalar_eval<POW_GENERAL>(v, sv, p, 0, out_std != nullptr, r, rs);
        }
        out_val[e] = r;
        if (out_std) out_std[e] = rs;
    }
    return HM_OK;
}

int hm_take_axis(const double* x, const double* s, double* out_val, double* out_std, int64_t outer, int64_t axis_len, int64_t inner,
                 const int64_t* indices, int n_indices, void*) {
    std::vector<int64_t> idx;
    if (const int rc = hm_rules::check_take_axis(x, s, out_val, out_std, outer, axis_len, inner, indices, n_indices, hm_rules::HOST,
                                                 [&] { idx.resize(static_cast<size_t>(n_indices)); return idx.data(); });
        rc != HM_OK) return rc;
    for (int64_t o = 0; o < outer; ++o)
        for (int q = 0; q < n_indices; ++q) {
            const int64_t src = (o * axis_len + idx[static_cast<size_t>(q)]) * inner, dst = (o * n_indices + q) * inner;
            std::memcpy(out_val + dst, x + src, static_cast<size_t>(inner) * 8u);
            if (out_std) std::memcpy(out_std + dst, s + src, static_cast<size_t>(inner) * 8u);
        }
    return HM_OK;
}

// ---- linearity statistics ----------------------------------------------------------------------------
int hm_apply_thresholds(double* val, double* std_, const double* lower, const double* upper, int64_t n, int C, void*) {
    if (const int rc = hm_rules::check_apply_thresholds(val, std_, lower, upper, n, C, hm_rules::HOST); rc != HM_OK) return rc;
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        const int c = static_cast<int>(e % C);
        const double v = val[e];
        if (v < lower[c] || v > upper[c]) { val[e] = kNaN; if (std_) std_[e] = kNaN; }                   // measurand.py:421-426
    }
    return HM_OK;
}

int hm_compute_difference_bcast(const double* x, const double* sx, const double* y, const double* sy, double multiplier, double* out_abs,
                                double* out_abs_std, double* out_rel, double* out_rel_std, int ndim, const int64_t* shape,
                                const int64_t* strides_x, const int64_t* strides_y, void*) {
    int64_t n;
    if (const int rc = hm_rules::check_compute_difference_bcast(x, sx, y, sy, out_abs, out_abs_std, out_rel, out_rel_std, ndim, shape, strides_x,
                                                            strides_y, n); rc != HM_OK) return rc;
    const bool with_std = sx || sy;
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        int64_t ox, oy;
        bcast_offsets(ndim, shape, strides_x, strides_y, e, ox, oy);
        double a, as = 0.0, r, rs = 0.0;
        diff_terms(x[ox], y[oy], sx ? sx[ox] : 0.0, sy ? sy[oy] : 0.0, multiplier, with_std, a, r, as, rs);
        out_abs[e] = a; out_rel[e] = r;
        if (with_std) { out_abs_std[e] = as; out_rel_std[e] = rs; }
    }
    return HM_OK;
}
int hm_compute_difference(const double* x, const double* sx, const double* y, const double* sy, double multiplier, double* out_abs,
                          double* out_abs_std, double* out_rel, double* out_rel_std, int64_t n, void* stream) {
    const int64_t shape[1] = {n}, st[1] = {1};                                       // n < 0: the negative extent of the _bcast rules
    return hm_compute_difference_bcast(x, sx, y, sy, multiplier, out_abs, out_abs_std, out_rel, out_rel_std, 1, shape, st, st, stream);
}

int hm_interpolate_bcast(const double* x0, const double* s0, const double* x1, const double* s1, double y0, double y1, double y,
                         double* out, double* out_std, int ndim, const int64_t* shape, const int64_t* strides0, const int64_t* strides1, void*) {
    int64_t n;
    if (const int rc = hm_rules::check_interpolate_bcast(x0, s0, x1, s1, out, out_std, ndim, shape, strides0, strides1, n); rc != HM_OK) return rc;
    const InterpCoef k = interp_coef(y0, y1, y);
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n; ++e) {
        int64_t o0, o1;
        bcast_offsets(ndim, shape, strides0, strides1, e, o0, o1);
        out[e] = interp_value(k, x0[o0], x1[o1]);
        if (out_std) out_std[e] = interp_std(k, s0 ? s0[o0] : 0.0, s1 ? s1[o1] : 0.0);
    }
    return HM_OK;
}
int hm_interpolate(const double* x0, const double* s0, const double* x1, const double* s1, double y0, double y1, double y, double* out,
                   double* out_std, int64_t n, void* stream) {
    const int64_t shape[1] = {n}, st[1] = {1};
    return hm_interpolate_bcast(x0, s0, x1, s1, y0, y1, y, out, out_std, 1, shape, st, st, stream);
}

size_t hm_axis_statistics_workspace_bytes(int64_t, int64_t, int64_t) { return 0; }
int hm_axis_statistics(const double* val, const double* std_, int64_t outer, int64_t axis_len, int64_t inner, double* out_mean,
                       double* out_std, double* out_err, void*, void*) {
    if (dense_elems({outer, axis_len, inner}) < 0 || !val || !out_mean || !out_std) return HM_EINVAL;
    if (!aligned8(val) || !aligned8(std_)) return HM_EALIGN;
    const int64_t n_out = outer * inner;
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < n_out; ++j) {
        const int64_t o = j / inner, i = j % inner;
        const double* pv = val + (o * axis_len) * inner + i;
        const double* ps = std_ ? std_ + (o * axis_len) * inner + i : nullptr;
        double mean, sd, err;
        line_statistics(axis_len, std_ != nullptr, [&](int64_t k, double& v, double& u) { v = pv[k * inner]; u = ps ? ps[k * inner] : 1.0; }, mean, sd, err);
        out_mean[j] = mean; out_std[j] = sd;
        if (out_err) out_err[j] = err;
    }
    return HM_OK;
}

size_t hm_axis_statistics2_workspace_bytes(int64_t, int64_t, int64_t, int64_t, int64_t) { return 0; }
int hm_axis_statistics2(const double* val, const double* std_, int64_t outer, int64_t a1, int64_t mid, int64_t a2, int64_t inner,
                        double* out_mean, double* out_std, double* out_err, void*, void*) {
    if (dense_elems({outer, a1, mid, a2, inner}) < 0 || !val || !out_mean || !out_std) return HM_EINVAL;
    if (!aligned8(val) || !aligned8(std_)) return HM_EALIGN;
    const int64_t n_out = outer * mid * inner, line = a1 * a2;
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < n_out; ++j) {
        const int64_t i = j % inner, m = (j / inner) % mid, o = j / (inner * mid);
        // element (o, k1, m, k2, i) of the dense (outer, a1, mid, a2, inner) block, line position k = k1 * a2 + k2 (NumPy's order of the reduced axes)
        auto at = [&](int64_t k) { return (((o * a1 + k / a2) * mid + m) * a2 + k % a2) * inner + i; };
        double mean, sd, err;
        line_statistics(line, std_ != nullptr, [&](int64_t k, double& v, double& u) { const int64_t e = at(k); v = val[e]; u = std_ ? std_[e] : 1.0; }, mean, sd, err);
        out_mean[j] = mean; out_std[j] = sd;
        if (out_err) out_err[j] = err;
    }
    return HM_OK;
}

size_t hm_channel_statistics_workspace_bytes(void) { return 64; }
int hm_channel_statistics(const double* val, const double* std_, int64_t n, int C, double* out, void* workspace, void*) {
    if (n < 1 || C < 1 || C > HM_MAX_CHANNELS || !val || !out || !workspace || n % C != 0) return HM_EINVAL;
    return hm_axis_statistics(val, std_, 1, n / C, C, out, out + C, out + 2 * C, nullptr, nullptr);
}

size_t hm_pair_statistics_workspace_bytes(void) { return 64; }
int hm_pair_statistics(const double* x, const double* sx, const double* y, const double* sy, double multiplier, int64_t n, int C,
                       double* out, void* workspace, void*) {
    if (n < 1 || C < 1 || C > HM_MAX_CHANNELS || !x || !y || !out || !workspace || n % C != 0) return HM_EINVAL;
    if (!aligned8(x) || !aligned8(y) || !aligned8(sx) || !aligned8(sy)) return HM_EALIGN;
    const bool with_std = sx || sy;
    const int64_t A = n / C;
    for (int h = 0; h < 2; ++h)
        for (int c = 0; c < C; ++c) {
            double mean, sd, err;
            line_statistics(A, with_std, [&](int64_t k, double& v, double& u) {
                const int64_t e = k * C + c;
                double a, as = 0.0, r, rs = 0.0;
                diff_terms(x[e], y[e], sx ? sx[e] : 0.0, sy ? sy[e] : 0.0, multiplier, with_std, a, r, as, rs);
                v = h == 0 ? a : r; u = h == 0 ? as : rs;
            }, mean, sd, err);
            double* o = out + 3 * C * h;
            o[c] = mean; o[C + c] = sd; o[2 * C + c] = err;
        }
    return HM_OK;
}

size_t hm_pairs_statistics_workspace_bytes(int) { return 64; }
int hm_pairs_statistics(const double* const* vals, const double* const* stds, int n_frames, const int32_t* pair_i, const int32_t* pair_j,
                        const double* multipliers, int n_pairs, int64_t n, int C, const double* lower, const double* upper, double* out,
                        void* workspace, void*) {
    const int rc = hm_rules::check_pairs(vals, stds, n_frames, pair_i, pair_j, multipliers, n_pairs, n, C, lower, upper, out, workspace);
    if (rc != HM_OK) return rc;
    if (lower)                                                                                           // exposure_series.py:437-441, in place
        for (int i = 0; i < n_frames; ++i)
            hm_apply_thresholds(const_cast<double*>(vals[i]), stds ? const_cast<double*>(stds[i]) : nullptr, lower, upper, n, C, nullptr);
#pragma omp parallel for schedule(dynamic)
    for (int p = 0; p < n_pairs; ++p)
        hm_pair_statistics(vals[pair_i[p]], stds ? stds[pair_i[p]] : nullptr, vals[pair_j[p]], stds ? stds[pair_j[p]] : nullptr, multipliers[p],
                           n, C, out + static_cast<int64_t>(p) * 6 * C, workspace, nullptr);
    return HM_OK;
}

// The same statistics straight from uint8 / uint16 DN frames: the thresholded per-(DN, channel) table first (pairs_dn_entry, the device
// build's formula), then hm_pair_statistics' loops on the mapped values. The frames are never written. `variant` places the table on the
// device; here it is only checked.
size_t hm_pairs_statistics_dn_workspace_bytes(int, int, int) { return 64; }
int hm_pairs_statistics_dn(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff,
                           const double* std_table, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                           int64_t n, int C, const double* lower, const double* upper, int variant, double* out, void* workspace, void*) {
    const int rc = hm_rules::check_pairs_dn(frames, n_frames, bit_depth, icrf, icrf_diff, std_table, pair_i, pair_j, multipliers, n_pairs, n, C,
                                            lower, upper, variant, out, workspace);
    if (rc != HM_OK) return rc;
    const bool with_std = std_table != nullptr;
    const int64_t entries = (int64_t{1} << bit_depth) * C;
    std::vector<double> tv(static_cast<size_t>(entries)), ts(static_cast<size_t>(with_std ? entries : 0));
    for (int64_t at = 0; at < entries; ++at) {
        const int c = static_cast<int>(at % C);
        double v, s;
        hm::pairs_dn_entry(icrf, icrf_diff, std_table, at, lower ? lower[c] : -kInf, upper ? upper[c] : kInf, v, s);
        tv[static_cast<size_t>(at)] = v;
        if (with_std) ts[static_cast<size_t>(at)] = s;
    }
    const uint32_t mask = (1u << bit_depth) - 1u;
    auto index = [&](const void* f, int64_t e) -> size_t {
        const uint32_t dn = bit_depth == 8 ? static_cast<const uint8_t*>(f)[e] : (static_cast<const uint16_t*>(f)[e] & mask);
        return static_cast<size_t>(dn) * C + static_cast<size_t>(e % C);
    };
    const int64_t A = n / C;
#pragma omp parallel for schedule(dynamic) collapse(2)
    for (int p = 0; p < n_pairs; ++p)
        for (int hc = 0; hc < 2 * C; ++hc) {
            const int h = hc / C, c = hc % C;
            const void* fx = frames[pair_i[p]];
            const void* fy = frames[pair_j[p]];
            double mean, sd, err;
            line_statistics(A, with_std, [&](int64_t k, double& v, double& u) {
                const int64_t e = k * C + c;
                const size_t ax = index(fx, e), ay = index(fy, e);
                double a, as = 0.0, r, rs = 0.0;
                diff_terms(tv[ax], tv[ay], with_std ? ts[ax] : 0.0, with_std ? ts[ay] : 0.0, multipliers[p], with_std, a, r, as, rs);
                v = h == 0 ? a : r; u = h == 0 ? as : rs;
            }, mean, sd, err);
            double* o = out + static_cast<int64_t>(p) * 6 * C + 3 * C * h;
            o[c] = mean; o[C + c] = sd; o[2 * C + c] = err;
        }
    return HM_OK;
}

int hm_pairs_statistics_dn_describe(int64_t n, int n_frames, int n_pairs, int C, int with_std, int bit_depth, int variant, int, char* buf,
                                    int buf_len) {
    if (!buf || buf_len < 1) return HM_EINVAL;
    buf[0] = '\0';
    const int rc = hm_rules::check_pairs_dn_counts(n_frames, n_pairs, n, C, with_std != 0, bit_depth, variant);
    if (rc != HM_OK) return rc;
    std::snprintf(buf, static_cast<size_t>(buf_len), "host_pairs_stats_dn<dn=%s,bits=%d,std=%d>", bit_depth == 8 ? "u8" : "u16", bit_depth, with_std != 0);
    return HM_OK;
}

size_t hm_histogram_workspace_bytes(int, int) { return 64; }
int hm_channel_minmax(const double* val, const double* std_, int64_t n, int C, double* out, void*, void*) {
    if (n < 1 || C < 1 || C > HM_MAX_CHANNELS || !val || !out) return HM_EINVAL;
    for (int c = 0; c < C; ++c) { out[2 * c] = kInf; out[2 * c + 1] = -kInf; }
    for (int64_t e = 0; e < n; ++e) {
        const double x = val[e];
        if (!hist_finite(x)) continue;
        if (std_ && std_[e] == 0.0) continue;
        const int c = static_cast<int>(e % C);
        out[2 * c] = std::fmin(out[2 * c], x); out[2 * c + 1] = std::fmax(out[2 * c + 1], x);
    }
    return HM_OK;
}
int hm_channel_histogram(const double* val, const double* std_, int64_t n, int C, int channel_mask, const double* edges, int bins, double lo,
                         double hi, double* out, void*, void*) {
    if (n < 1 || C < 1 || C > HM_MAX_CHANNELS || bins < 1 || !val || !edges || !out || !(hi > lo)) return HM_EINVAL;
    if (static_cast<int64_t>(bins) * C > 8192) return HM_EUNSUPPORTED;         // (the device build's limit, 64 KB of LDS: one ABI, one answer)
    for (int i = 0; i < C * bins; ++i) out[i] = 0.0;
    const double norm = static_cast<double>(bins) / (hi - lo);
    for (int64_t e = 0; e < n; ++e) {                                                                     // np.histogram, measurand.py:430-469
        const int c = static_cast<int>(e % C);
        if (!((channel_mask >> c) & 1)) continue;
        const double x = val[e];
        if (!hist_finite(x)) continue;
        double w = 1.0;
        if (std_ && !hist_weight(std_[e], w)) continue;
        if (!hist_in_range(x, lo, hi)) continue;
        out[c * bins + hist_bin(x, lo, norm, edges, bins)] += w;
    }
    return HM_OK;
}

// ---- distributions of all exposure pairs (hm_pairs_minmax / hm_pairs_histogram): the difference terms of diff_terms() on the values as
// read through the thresholds, hm_channel_minmax's / hm_channel_histogram's counting rule, weighted sums added in index order. The same
// loops serve hm_pairs_minmax_dn / hm_pairs_histogram_dn on the values a thresholded per-(DN, channel) table maps the DN frames to.
}  // extern "C" (the loops are templates over the element source)
namespace {
// element e of pair (x, y): loaded, thresholded as read (a value outside its channel's limits is NaN with its std), differenced
struct PairElems {
    const double* x; const double* sx; const double* y; const double* sy;
    const double* lower; const double* upper;
    double mult; int C;
    void at(int64_t e, double& a, double& as, double& r, double& rs) const {
        double xv = x[e], yv = y[e], xs = sx ? sx[e] : 0.0, ys = sy ? sy[e] : 0.0;
        if (lower) {
            const int c = static_cast<int>(e % C);
            if (xv < lower[c] || xv > upper[c]) { xv = kNaN; xs = sx ? kNaN : 0.0; }                      // measurand.py:418
            if (yv < lower[c] || yv > upper[c]) { yv = kNaN; ys = sy ? kNaN : 0.0; }
        }
        as = 0.0; rs = 0.0;
        diff_terms(xv, yv, xs, ys, mult, sx != nullptr, a, r, as, rs);
    }
};

// The thresholded table of the DN entries (pairs_dn_entry, the device build's formula) and element e of a pair of DN frames through it.
struct PairsDnTable {
    std::vector<double> tv, ts;
    int bit_depth, C; bool with_std; uint32_t mask;
    PairsDnTable(const double* icrf, const double* icrf_diff, const double* std_table, const double* lower, const double* upper, int bit_depth_,
                 int C_) : bit_depth(bit_depth_), C(C_), with_std(std_table != nullptr), mask((1u << bit_depth_) - 1u) {
        const int64_t entries = (int64_t{1} << bit_depth) * C;
        tv.resize(static_cast<size_t>(entries)); ts.resize(static_cast<size_t>(with_std ? entries : 0));
        for (int64_t at = 0; at < entries; ++at) {
            const int c = static_cast<int>(at % C);
            double v, s;
            hm::pairs_dn_entry(icrf, icrf_diff, std_table, at, lower ? lower[c] : -kInf, upper ? upper[c] : kInf, v, s);
            tv[static_cast<size_t>(at)] = v;
            if (with_std) ts[static_cast<size_t>(at)] = s;
        }
    }
    size_t index(const void* f, int64_t e) const {
        const uint32_t dn = bit_depth == 8 ? static_cast<const uint8_t*>(f)[e] : (static_cast<const uint16_t*>(f)[e] & mask);
        return static_cast<size_t>(dn) * C + static_cast<size_t>(e % C);
    }
};
struct PairDnElems {
    const PairsDnTable* t; const void* fx; const void* fy; double mult;
    void at(int64_t e, double& a, double& as, double& r, double& rs) const {
        const size_t ax = t->index(fx, e), ay = t->index(fy, e);
        as = 0.0; rs = 0.0;
        diff_terms(t->tv[ax], t->tv[ay], t->with_std ? t->ts[ax] : 0.0, t->with_std ? t->ts[ay] : 0.0, mult, t->with_std, a, r, as, rs);
    }
};

// pair(p) -> the element source of pair p (PairElems, PairDnElems)
template <class Pair>
void pairs_minmax_loop(Pair pair, int n_pairs, int64_t n, int C, bool weighted, double* out) {
#pragma omp parallel for schedule(dynamic)
    for (int p = 0; p < n_pairs; ++p) {
        const auto pe = pair(p);
        double* o = out + static_cast<int64_t>(p) * 2 * C * 2;
        for (int i = 0; i < 2 * C; ++i) { o[2 * i] = kInf; o[2 * i + 1] = -kInf; }
        for (int64_t e = 0; e < n; ++e) {
            double v[2], s[2];
            pe.at(e, v[0], s[0], v[1], s[1]);
            const int c = static_cast<int>(e % C);
            for (int k = 0; k < 2; ++k) {
                if (!hist_finite(v[k])) continue;
                if (weighted && s[k] == 0.0) continue;
                double* m = o + (k * C + c) * 2;
                m[0] = std::fmin(m[0], v[k]); m[1] = std::fmax(m[1], v[k]);
            }
        }
    }
}
template <class Pair>
void pairs_histogram_loop(Pair pair, int n_pairs, int64_t n, int C, int channel_mask, bool weighted, const double* edges, int bins, double* out) {
#pragma omp parallel for schedule(dynamic)
    for (int p = 0; p < n_pairs; ++p) {
        const auto pe = pair(p);
        double* o = out + static_cast<int64_t>(p) * 2 * C * bins;
        const double* eg = edges + static_cast<int64_t>(p) * 2 * C * (bins + 1);
        for (int64_t i = 0; i < int64_t{2} * C * bins; ++i) o[i] = 0.0;
        for (int64_t e = 0; e < n; ++e) {
            const int c = static_cast<int>(e % C);
            if (!((channel_mask >> c) & 1)) continue;
            double v[2], s[2];
            pe.at(e, v[0], s[0], v[1], s[1]);
            for (int k = 0; k < 2; ++k) {
                const double x = v[k];
                const double* ek = eg + static_cast<int64_t>(k * C + c) * (bins + 1);
                const double lo = ek[0], hi = ek[bins];
                if (!(hi > lo)) continue;                                                                 // (hm_channel_histogram: HM_EINVAL)
                if (!hist_finite(x)) continue;
                double w = 1.0;
                if (weighted && !hist_weight(s[k], w)) continue;
                if (!hist_in_range(x, lo, hi)) continue;
                o[static_cast<int64_t>(k * C + c) * bins + hist_bin_bounded(x, lo, static_cast<double>(bins) / (hi - lo), ek, bins)] += w;
            }
        }
    }
}
}  // namespace
extern "C" {

size_t hm_pairs_histogram_workspace_bytes(int, int, int) { return 64; }
int hm_pairs_minmax(const double* const* vals, const double* const* stds, int n_frames, const int32_t* pair_i, const int32_t* pair_j,
                    const double* multipliers, int n_pairs, int64_t n, int C, const double* lower, const double* upper, double* out,
                    void* workspace, void*) {
    const int rc = hm_rules::check_pairs(vals, stds, n_frames, pair_i, pair_j, multipliers, n_pairs, n, C, lower, upper, out, workspace);
    if (rc != HM_OK) return rc;
    pairs_minmax_loop([&](int p) {
        return PairElems{vals[pair_i[p]], stds ? stds[pair_i[p]] : nullptr, vals[pair_j[p]], stds ? stds[pair_j[p]] : nullptr, lower, upper,
                         multipliers[p], C};
    }, n_pairs, n, C, stds != nullptr, out);
    return HM_OK;
}
int hm_pairs_histogram(const double* const* vals, const double* const* stds, int n_frames, const int32_t* pair_i, const int32_t* pair_j,
                       const double* multipliers, int n_pairs, int64_t n, int C, int channel_mask, const double* lower, const double* upper,
                       const double* edges, int bins, double* out, void* workspace, void*) {
    const int rc = hm_rules::check_pairs_histogram(vals, stds, n_frames, pair_i, pair_j, multipliers, n_pairs, n, C, channel_mask, lower, upper,
                                                   edges, bins, out, workspace);
    if (rc != HM_OK) return rc;
    pairs_histogram_loop([&](int p) {
        return PairElems{vals[pair_i[p]], stds ? stds[pair_i[p]] : nullptr, vals[pair_j[p]], stds ? stds[pair_j[p]] : nullptr, lower, upper,
                         multipliers[p], C};
    }, n_pairs, n, C, channel_mask, stds != nullptr, edges, bins, out);
    return HM_OK;
}

// The same distributions straight from uint8 / uint16 DN frames: the table first, then the loops above on the mapped values. The frames
// are never written. `variant` places the table on the device; here it is only checked (the fit rule: hm_pairs_rules.h).
size_t hm_pairs_histogram_dn_workspace_bytes(int, int, int, int) { return 64; }
int hm_pairs_minmax_dn(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff,
                       const double* std_table, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs, int64_t n,
                       int C, const double* lower, const double* upper, int variant, double* out, void* workspace, void*) {
    const int rc = hm_rules::check_pairs_minmax_dn(frames, n_frames, bit_depth, icrf, icrf_diff, std_table, pair_i, pair_j, multipliers, n_pairs,
                                                   n, C, lower, upper, variant, out, workspace);
    if (rc != HM_OK) return rc;
    const PairsDnTable t(icrf, icrf_diff, std_table, lower, upper, bit_depth, C);
    pairs_minmax_loop([&](int p) { return PairDnElems{&t, frames[pair_i[p]], frames[pair_j[p]], multipliers[p]}; }, n_pairs, n, C, t.with_std, out);
    return HM_OK;
}
int hm_pairs_histogram_dn(const void* const* frames, int n_frames, int bit_depth, const double* icrf, const double* icrf_diff,
                          const double* std_table, const int32_t* pair_i, const int32_t* pair_j, const double* multipliers, int n_pairs,
                          int64_t n, int C, int channel_mask, const double* lower, const double* upper, const double* edges, int bins,
                          int variant, double* out, void* workspace, void*) {
    const int rc = hm_rules::check_pairs_histogram_dn(frames, n_frames, bit_depth, icrf, icrf_diff, std_table, pair_i, pair_j, multipliers,
                                                      n_pairs, n, C, channel_mask, lower, upper, edges, bins, variant, out, workspace);
    if (rc != HM_OK) return rc;
    const PairsDnTable t(icrf, icrf_diff, std_table, lower, upper, bit_depth, C);
    pairs_histogram_loop([&](int p) { return PairDnElems{&t, frames[pair_i[p]], frames[pair_j[p]], multipliers[p]}; }, n_pairs, n, C,
                         channel_mask, t.with_std, edges, bins, out);
    return HM_OK;
}
int hm_pairs_histogram_dn_describe(int64_t n, int n_frames, int n_pairs, int C, int with_std, int bit_depth, int bins, int variant, char* buf,
                                   int buf_len) {
    if (!buf || buf_len < 1) return HM_EINVAL;
    buf[0] = '\0';
    const int rc = hm_rules::check_pairs_hist_dn_counts(n_frames, n_pairs, n, C, with_std != 0, bit_depth, bins, variant);
    if (rc != HM_OK) return rc;
    std::snprintf(buf, static_cast<size_t>(buf_len), "host_pairs_hist_dn<dn=%s,bits=%d,std=%d>", bit_depth == 8 ? "u8" : "u16", bit_depth, with_std != 0);
    return HM_OK;
}

}  // extern "C" (templates below)
// ---- the producers ---------------------------------------------------------------------------------
// welford_algorithm, modules/video_processing.py:161-219: per element, frames in order - delta = f - mean; mean += delta / n;
// m2 += delta * (f - mean) (:205-208), f = icrf[dn, c] (:200-201) or dn / 255 (:203). One text for uint8 frames (mask 255, max_dn 255.0)
// and uint16 frames of 9 to 16 bits (mask = max_dn = 2^bit_depth - 1): f = icrf[DN & mask, c] or (DN & mask) / max_dn.
template <typename DN>
static void welford_update(const void* const* frames, int n_frames, int64_t count_before, const double* icrf, double* mean, double* m2,
                           int64_t n_elems, int C, int mask, double max_dn) {
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n_elems; ++e) {
        const int c = static_cast<int>(e % C);
        double m = mean[e], q = m2 ? m2[e] : 0.0, cnt = static_cast<double>(count_before);
        for (int k = 0; k < n_frames; ++k) {
            cnt += 1.0;
            const int dn = static_cast<const DN*>(frames[k])[e] & mask;
            const double f = icrf ? icrf[dn * C + c] : static_cast<double>(dn) / max_dn;
            const double delta = f - m;
            m = m + delta / cnt;
            q = q + delta * (f - m);
        }
        mean[e] = m;
        if (m2) m2[e] = q;
    }
}

// mean -> around(mean * max_dn) (:210-211), std -> around(sqrt(m2 / (n - 1)) / sqrt(n)) (:214-215, as written: not rescaled)
template <typename DN>
static void welford_finalize(const double* mean, const double* m2, int64_t count, double max_dn, DN* out_mean, DN* out_std, int64_t n_elems) {
    const double denom = static_cast<double>(count) - 1.0, root_n = std::sqrt(static_cast<double>(count));
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < n_elems; ++e) {
        if (out_mean) out_mean[e] = round_to_dn<DN>(mean[e] * max_dn);
        if (out_std) out_std[e] = round_to_dn<DN>(std::sqrt(m2[e] / denom) / root_n);
    }
}

extern "C" {
int hm_welford_update(const void* const* frames, int n_frames, int64_t count_before, const double* icrf, double* mean, double* m2,
                      int64_t n_elems, int C, void*) {
    bool empty;
    const int rc = hm_rules::check_welford_update(frames, n_frames, count_before, mean, n_elems, C, empty);
    if (rc != HM_OK || empty) return rc;
    welford_update<uint8_t>(frames, n_frames, count_before, icrf, mean, m2, n_elems, C, 255, 255.0);
    return HM_OK;
}

int hm_welford_finalize(const double* mean, const double* m2, int64_t count, uint8_t* out_mean, uint8_t* out_std, int64_t n_elems, void*) {
    bool empty;
    const int rc = hm_rules::check_welford_finalize(mean, m2, count, out_mean, out_std, n_elems, empty);
    if (rc != HM_OK || empty) return rc;
    welford_finalize<uint8_t>(mean, m2, count, 255.0, out_mean, out_std, n_elems);
    return HM_OK;
}
int64_t hm_welford_algorithmic_bytes(int n_frames, int with_m2, int64_t n_elems) {
    return hm_rules::welford_algorithmic_bytes(1, n_frames, with_m2 != 0, n_elems);
}

// ... on uint16 frames of 9 to 16 bits, M = 2^bit_depth - 1. `variant` places the table on the device; here it is only checked.
int hm_welford_update_u16(const void* const* frames, int n_frames, int64_t count_before, const double* icrf, double* mean, double* m2,
                          int64_t n_elems, int C, int bit_depth, int variant, void*) {
    bool empty;
    const int rc = hm_rules::check_welford_update_u16(frames, n_frames, count_before, icrf, mean, n_elems, C, bit_depth, variant, empty);
    if (rc != HM_OK || empty) return rc;
    const int mask = (1 << bit_depth) - 1;
    welford_update<uint16_t>(frames, n_frames, count_before, icrf, mean, m2, n_elems, C, mask, static_cast<double>(mask));
    return HM_OK;
}

int hm_welford_update_u16_describe(int64_t n_elems, int n_frames, int C, int with_icrf, int with_m2, int bit_depth, int variant, char* buf,
                                   int buf_len) {
    if (!buf || buf_len < 1) return HM_EINVAL;
    buf[0] = '\0';
    bool empty;
    const int rc = hm_rules::check_welford_update_u16_counts(n_frames, 0, n_elems, C, with_icrf != 0, bit_depth, variant, empty);
    if (rc != HM_OK || empty) return rc;
    std::snprintf(buf, static_cast<size_t>(buf_len), "host_welford<dn=u16,m2=%d,icrf=%d,bits=%d>", with_m2 != 0, with_icrf != 0, bit_depth);
    return HM_OK;
}

int hm_welford_finalize_u16(const double* mean, const double* m2, int64_t count, int bit_depth, uint16_t* out_mean, uint16_t* out_std,
                            int64_t n_elems, void*) {
    bool empty;
    const int rc = hm_rules::check_welford_finalize_u16(mean, m2, count, bit_depth, out_mean, out_std, n_elems, empty);
    if (rc != HM_OK || empty) return rc;
    welford_finalize<uint16_t>(mean, m2, count, static_cast<double>((1 << bit_depth) - 1), out_mean, out_std, n_elems);
    return HM_OK;
}
int64_t hm_welford_u16_algorithmic_bytes(int n_frames, int with_m2, int64_t n_elems) {
    return hm_rules::welford_algorithmic_bytes(2, n_frames, with_m2 != 0, n_elems);
}

// compute_noise_profiles, modules/video_processing.py:77-106: profile[m, f, c] += 1 for every frame and element (np.add.at).
// Per thread a private (256, 256, C) count over its elements, added into the profile at the end: exact, any thread count.
size_t hm_noise_profile_workspace_bytes(int64_t, int) { return 0; }
int64_t hm_noise_profile_algorithmic_bytes(int n_frames, int64_t n_elems, int C) {
    return n_elems * (static_cast<int64_t>(n_frames) + 1) + int64_t{2} * 256 * 256 * C * 8;
}
int hm_noise_profile_update(const void* const* frames, int n_frames, const uint8_t* mean, int64_t n_elems, int C, int64_t* profiles,
                            void*, int64_t workspace_bytes, void*) {
    bool empty;
    const int rc = hm_rules::check_noise_profile_update(frames, n_frames, mean, n_elems, C, profiles, workspace_bytes, empty);
    if (rc != HM_OK || empty) return rc;
#pragma omp parallel
    {
        std::vector<int64_t> loc(static_cast<size_t>(256) * 256 * C, 0);
#pragma omp for schedule(static)
        for (int64_t e = 0; e < n_elems; ++e) {
            int64_t* row = loc.data() + (static_cast<int64_t>(mean[e]) * 256 * C + e % C);
            for (int k = 0; k < n_frames; ++k) row[static_cast<int64_t>(static_cast<const uint8_t*>(frames[k])[e]) * C] += 1;
        }
#pragma omp critical
        for (size_t i = 0; i < loc.size(); ++i) profiles[i] += loc[i];
    }
    return HM_OK;
}

// _calculate_STD, video_processing.py:109-133, per (level i, channel c): over the non-zero bins h of row i with edges
// linspace(0, 1, 256) (the caller's table), mean = sum(h * edges) / sum(h), std = sqrt(sum((edges - mean)^2 h) / sum(h));
// an empty row gives 0 / 0 = NaN (math.sqrt of NaN: the documented deviation of the Python layer)
int hm_noise_profile_std(const int64_t* profiles, int C, const double* edges, double* out_std, void*) {
    const int rc = hm_rules::check_noise_profile_std(profiles, C, edges, out_std);
    if (rc != HM_OK) return rc;
#pragma omp parallel for schedule(static)
    for (int t = 0; t < 256 * C; ++t) {
        const int i = t / C, c = t % C;
        const int64_t* row = profiles + static_cast<int64_t>(i) * 256 * C + c;
        double cnt = 0.0, s1 = 0.0;
        for (int b = 0; b < 256; ++b) {
            const double h = static_cast<double>(row[b * C]);
            if (h != 0.0) { cnt += h; s1 += h * edges[b]; }
        }
        const double mean = s1 / cnt;
        double s2 = 0.0;
        for (int b = 0; b < 256; ++b) {
            const double h = static_cast<double>(row[b * C]);
            if (h != 0.0) { const double dv = edges[b] - mean; s2 += (dv * dv) * h; }
        }
        out_std[i * C + c] = std::sqrt(s2 / cnt);
    }
    return HM_OK;
}

// clean_data_edges, video_processing.py:12-74: per (row i, channel c) the four integer passes centred at i, in order, in place
int hm_noise_profile_clean_edges(int64_t* profiles, int C, void*) {
    const int rc = hm_rules::check_noise_profile_clean_edges(profiles, C);
    if (rc != HM_OK) return rc;
#pragma omp parallel for schedule(static)
    for (int t = 0; t < 256 * C; ++t) {
        const int i = t / C, c = t % C;
        int64_t* row = profiles + static_cast<int64_t>(i) * 256 * C + c;
        clean_edges_row([&](int m) -> int64_t& { return row[static_cast<int64_t>(m) * C]; }, i);
    }
    return HM_OK;
}

// The per-level noise moments of uint16 frames of 9 to 16 bits, M = 2^bit_depth - 1: per element the sums of d = f - m over the frames,
// then one add per element into moments[m][c][0..2]; unsigned arithmetic, modulo 2^64 as the header states. `variant` places the table on
// the device; here it is only checked.
int64_t hm_noise_moments_algorithmic_bytes(int n_frames, int64_t n_elems, int C, int bit_depth) {
    return hm_rules::noise_moments_algorithmic_bytes(n_frames, n_elems, C, bit_depth);
}
int hm_noise_moments_update_u16(const void* const* frames, int n_frames, const uint16_t* mean, int64_t n_elems, int C, int bit_depth,
                                int64_t* moments, int variant, void*) {
    bool empty;
    const int rc = hm_rules::check_noise_moments_update(frames, n_frames, mean, n_elems, C, bit_depth, moments, variant, empty);
    if (rc != HM_OK || empty) return rc;
    const uint32_t mask = (1u << bit_depth) - 1u;
    uint64_t* mom = reinterpret_cast<uint64_t*>(moments);
    for (int64_t e = 0; e < n_elems; ++e) {
        const uint32_t m = mean[e] & mask;
        uint64_t s1 = 0, s2 = 0;
        for (int k = 0; k < n_frames; ++k) {
            const int64_t d = static_cast<int64_t>(static_cast<const uint16_t*>(frames[k])[e] & mask) - static_cast<int64_t>(m);
            s1 += static_cast<uint64_t>(d);
            s2 += static_cast<uint64_t>(d * d);
        }
        uint64_t* t = mom + (static_cast<int64_t>(m) * C + e % C) * 3;
        t[0] += static_cast<uint64_t>(n_frames);
        t[1] += s1;
        t[2] += s2;
    }
    return HM_OK;
}
int hm_noise_moments_update_u16_describe(int64_t n_elems, int n_frames, int C, int bit_depth, int variant, char* buf, int buf_len) {
    if (!buf || buf_len < 1) return HM_EINVAL;
    buf[0] = '\0';
    const int rc = hm_rules::check_noise_moments_update_counts(n_frames, n_elems, C, bit_depth, variant);
    if (rc != HM_OK || n_frames == 0 || n_elems == 0) return rc;
    std::snprintf(buf, static_cast<size_t>(buf_len), "host_noise_moments<dn=u16,C=%d,bits=%d>", C, bit_depth);
    return HM_OK;
}
int hm_noise_moments_std(const int64_t* moments, int C, int bit_depth, double* out_std, void*) {
    const int rc = hm_rules::check_noise_moments_std(moments, C, bit_depth, out_std);
    if (rc != HM_OK) return rc;
    const int n_ent = (1 << bit_depth) * C;
    const double max_dn = static_cast<double>((1 << bit_depth) - 1);
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n_ent; ++i) {
        const int64_t* t = moments + static_cast<int64_t>(i) * 3;
        out_std[i] = noise_moments_level_std(t[0], t[1], t[2], max_dn);
    }
    return HM_OK;
}

// compute_kernel_density_estimate, modules/measurand.py:716-761 (gaussian_kde(values, 'silverman', weights).evaluate), one channel.
// The operation sequence of hm_kde.hip: counted = finite x (and std != 0), w = 1 / std or 1; moments over kKdeSlices fixed slices
// added in order (the same bits for any thread count); evaluate sums w exp(-(d * d) * 0.5), d = x / h - y / h, per chunk of
// kKdeChunk elements, the chunks in order, times `scale`.
constexpr int kKdeSlices = 256;
constexpr int64_t kKdeChunk = 4096;
size_t hm_kde_workspace_bytes(int64_t, int, int) { return 0; }
int hm_kde_moments(const double* val, const double* std_, int64_t n_elems, int C, int channel, double* moments, void*, int64_t workspace_bytes, void*) {
    const int rc = hm_rules::check_kde_moments(val, n_elems, C, channel, moments, nullptr, workspace_bytes, false);
    if (rc != HM_OK) return rc;
    const int64_t n = n_elems / C;
    std::vector<double> part(static_cast<size_t>(kKdeSlices) * 10);
#pragma omp parallel for schedule(static)
    for (int s = 0; s < kKdeSlices; ++s) {
        double v[9] = {0.0, 0.0, 0.0, 0.0, kInf, -kInf, 0.0, 0.0, 0.0};
        for (int64_t i = n * s / kKdeSlices; i < n * (s + 1) / kKdeSlices; ++i) {
            double x, w;
            if (!kde_load(val, std_, i * C + channel, x, w)) continue;
            v[0] += 1.0; v[1] += w; v[2] += w * w; v[3] += w * x;
            v[4] = std::fmin(v[4], x); v[5] = std::fmax(v[5], x);
            v[6] += std::isfinite(w) ? 0.0 : 1.0; v[7] += w > 0.0 ? 1.0 : 0.0; v[8] += w < 0.0 ? 1.0 : 0.0;
        }
        std::copy(v, v + 9, part.begin() + s * 10);
    }
    double r[9] = {0.0, 0.0, 0.0, 0.0, kInf, -kInf, 0.0, 0.0, 0.0};
    for (int s = 0; s < kKdeSlices; ++s)
        for (int k = 0; k < 9; ++k) {
            const double o = part[s * 10 + k];
            r[k] = k == 4 ? std::fmin(r[k], o) : k == 5 ? std::fmax(r[k], o) : r[k] + o;
        }
    const double xbar = r[3] / r[1];
#pragma omp parallel for schedule(static)
    for (int s = 0; s < kKdeSlices; ++s) {
        double a = 0.0;
        for (int64_t i = n * s / kKdeSlices; i < n * (s + 1) / kKdeSlices; ++i) {
            double x, w;
            if (!kde_load(val, std_, i * C + channel, x, w)) continue;
            const double d = x - xbar;
            a += w * (d * d);
        }
        part[s * 10] = a;
    }
    double m2 = 0.0;
    for (int s = 0; s < kKdeSlices; ++s) m2 += part[s * 10];
    std::copy(r, r + 9, moments);
    moments[9] = xbar;
    moments[10] = m2;
    return HM_OK;
}
int hm_kde_evaluate(const double* val, const double* std_, int64_t n_elems, int C, int channel, double h, double scale, const double* grid,
                    int m, double* out, void*, int64_t workspace_bytes, void*) {
    bool empty;
    const int rc = hm_rules::check_kde_evaluate(val, n_elems, C, channel, h, scale, grid, m, out, nullptr, workspace_bytes, false, empty);
    if (rc != HM_OK || empty) return rc;
    const int64_t n = n_elems / C;
    std::vector<double> u, w;                                        // the counted elements, u = x / h
    for (int64_t i = 0; i < n; ++i) {
        double x, wi;
        if (kde_load(val, std_, i * C + channel, x, wi)) { u.push_back(x / h); w.push_back(wi); }
    }
    const int64_t nc = static_cast<int64_t>(u.size());
#pragma omp parallel for schedule(static)
    for (int j = 0; j < m; ++j) {
        const double v = grid[j] / h;
        double total = 0.0;
        for (int64_t k0 = 0; k0 < nc; k0 += kKdeChunk) {
            double acc = 0.0;
            const int64_t k1 = std::min(nc, k0 + kKdeChunk);
            for (int64_t k = k0; k < k1; ++k) {
                const double d = u[k] - v;
                acc += w[k] * std::exp(-(d * d) * 0.5);
            }
            total += acc;
        }
        out[j] = total * scale;
    }
    return HM_OK;
}

}  // extern "C" (a template below)

// _energy_function + analyze_linearity, modules/ICRF_calibration_exposure.py:66-145,148-201, for n_candidates ICRFs of one channel:
// per candidate and exposure pair (i < j, np.triu_indices order) the (weighted) mean of |v_i - v_j t_i/t_j| (/ (v_j t_i/t_j) when
// relative) over the pixels whose values lie inside [icrf[lower], icrf[upper]]; the energy is the nanmean over the pairs, +inf for NaN
// (validated arguments) DN: uint8_t with n_rows = 256 (hm_linearity_energy), uint16_t with n_rows = 2^bit_depth (hm_linearity_energy_u16);
// a DN's index is DN & (n_rows - 1) - every uint8 DN is its own
template <typename DN>
static int linearity_energy_host(const DN* dn, const double* std_, const double* exposures, const double* icrf, const uint8_t* valid,
                                 int n_candidates, int lower, int upper, int use_relative, int64_t n_pixels, int n_frames, int n_rows,
                                 double* out_pairs, double* out_energy) {
    const unsigned mask = static_cast<unsigned>(n_rows - 1);
    const int N = n_frames, pairs = N * (N - 1) / 2;
    std::vector<int> pi(pairs), pj(pairs);
    { int p = 0; for (int i = 0; i < N; ++i) for (int j = i + 1; j < N; ++j, ++p) { pi[p] = i; pj[p] = j; } }
    std::vector<double> res(static_cast<size_t>(n_candidates) * pairs);
#pragma omp parallel for collapse(2) schedule(dynamic)
    for (int b = 0; b < n_candidates; ++b)
        for (int p = 0; p < pairs; ++p) {
            double& r = res[static_cast<size_t>(b) * pairs + p];
            if (valid && !valid[b]) { r = kNaN; continue; }
            const double* lut = icrf + static_cast<int64_t>(b) * n_rows;
            const double lo = lut[lower], hi = lut[upper];
            const int i = pi[p], j = pj[p];
            const double ratio = exposures[i] / exposures[j];                            // :100
            double num = 0.0, den = 0.0, bnum = 0.0, bden = 0.0;                       // sums in blocks of 1024 pixels (a million-term running sum
            for (int64_t px = 0; px < n_pixels; ++px) {                                  // loses three more digits than NumPy's pairwise one)
                if ((px & 1023) == 0) { num += bnum; den += bden; bnum = 0.0; bden = 0.0; }
                double vi = lut[dn[px * N + i] & mask], vj = lut[dn[px * N + j] & mask];
                if (vi < lo || vi > hi) vi = kNaN;                                       // :96-97
                if (vj < lo || vj > hi) vj = kNaN;
                const double scaled = vj * ratio;                                        // :111
                double d = vi - scaled;                                                  // :114
                if (use_relative) d = d / scaled;                                        // :117
                const double ad = std::fabs(d);                                          // :120
                if (std_) {
                    const double si = std_[px * N + i], sj = std_[px * N + j];
                    double sigma;
                    if (use_relative) {
                        const double u = si / scaled, v = (vi * sj) / (ratio * (vj * vj));   // :127
                        sigma = std::sqrt(u * u + v * v);
                    } else {
                        const double v = ratio * sj;
                        sigma = std::sqrt(si * si + v * v);                              // :129
                    }
                    const double w = 1.0 / sigma;
                    if (std::isfinite(ad) && sigma != 0.0 && w == w) { bnum += ad * w; bden += w; }   // :133-134, general_functions.py:164-174
                } else if (ad == ad) { bnum += ad; bden += 1.0; }                        // :138
            }
            num += bnum; den += bden;
            r = num / den;                                                               // 0 / 0 = NaN: no contributing pixel
        }
    for (int b = 0; b < n_candidates; ++b) {
        const bool ok = !valid || valid[b];
        double sum = 0.0, cnt = 0.0;
        for (int p = 0; p < pairs; ++p) {
            const double r = res[static_cast<size_t>(b) * pairs + p];
            if (out_pairs) out_pairs[static_cast<int64_t>(b) * pairs + p] = r;
            if (r == r) { sum += r; cnt += 1.0; }
        }
        const double e = sum / cnt;                                                      // :196
        out_energy[b] = (ok && e == e) ? e : std::numeric_limits<double>::infinity();    // :197-200
    }
    return HM_OK;
}

extern "C" {

size_t hm_linearity_energy_workspace_bytes(int64_t, int, int) { return 0; }
int hm_linearity_energy(const uint8_t* dn, const double* std_, const double* exposures, const double* icrf, const uint8_t* valid,
                        int n_candidates, int lower, int upper, int use_relative, int64_t n_pixels, int n_frames,
                        double* out_pairs, double* out_energy, void*, void*) {
    bool empty;
    const int rc = hm_rules::check_linearity_energy(dn, exposures, icrf, n_candidates, lower, upper, n_pixels, n_frames, out_energy, empty);
    if (rc != HM_OK || empty) return rc;
    return linearity_energy_host(dn, std_, exposures, icrf, valid, n_candidates, lower, upper, use_relative, n_pixels, n_frames, 256, out_pairs,
                                 out_energy);
}

// ... on uint16 DNs of 9 to 16 bits, candidate rows of 2^bit_depth entries. `variant` places the row on the device; here it is only checked.
int hm_linearity_energy_u16(const uint16_t* dn, const double* std_, const double* exposures, const double* icrf, const uint8_t* valid,
                            int n_candidates, int lower, int upper, int use_relative, int64_t n_pixels, int n_frames, int bit_depth,
                            int variant, double* out_pairs, double* out_energy, void*, void*) {
    bool empty;
    const int rc = hm_rules::check_linearity_energy_u16(dn, exposures, icrf, n_candidates, lower, upper, n_pixels, n_frames, bit_depth, variant,
                                                        out_energy, empty);
    if (rc != HM_OK || empty) return rc;
    return linearity_energy_host(dn, std_, exposures, icrf, valid, n_candidates, lower, upper, use_relative, n_pixels, n_frames, 1 << bit_depth,
                                 out_pairs, out_energy);
}

int hm_linearity_energy_u16_describe(int64_t n_pixels, int n_frames, int n_candidates, int with_std, int bit_depth, int variant, char* buf,
                                     int buf_len) {
    if (!buf || buf_len < 1) return HM_EINVAL;
    buf[0] = '\0';
    bool empty;
    const int rc = hm_rules::check_linearity_energy_u16_counts(n_candidates, 0, 0, n_pixels, n_frames, bit_depth, variant, empty);
    if (rc != HM_OK || empty) return rc;
    std::snprintf(buf, static_cast<size_t>(buf_len), "host_linearity_energy<dn=u16,std=%d,bits=%d>(N=%d)", with_std != 0, bit_depth, n_frames);
    return HM_OK;
}

// One generation of the ICRF-calibration differential evolution (calibration(), modules/ICRF_calibration_exposure.py:288-369), as
// specified in hdrmerge.h: trial (mutation, crossover, redraw), candidate ICRF + verdicts, energy (hm_linearity_energy above),
// deferred selection, statistics and the stop flag - the HIP build's hm_de.hip with host pointers.
static inline double de_tree_sum(std::vector<double>& v) {                // the HIP build's fixed-order tree (size: a power of two)
    for (size_t s = v.size() >> 1; s > 0; s >>= 1)
        for (size_t t = 0; t < s; ++t) v[t] += v[t + s];
    return v[0];
}

// the select stage of a generation g (k_de_select): deferred selection, best index / mean / std, the stop flag, the generation counter
static void de_select_host(double* population, double* energies, const double* trial, const double* trial_energies, int64_t* status,
                           int S, int P, int64_t g, int64_t max_generations, double tol, double energy_limit) {
    size_t n = 1;
    while (n < static_cast<size_t>(S)) n <<= 1;
    std::vector<double> v(n, 0.0);
    for (int i = 0; i < S; ++i) {
        if (g == 0 || trial_energies[i] <= energies[i]) {
            energies[i] = trial_energies[i];
            std::memcpy(population + static_cast<int64_t>(i) * P, trial + static_cast<int64_t>(i) * P, sizeof(double) * P);
        }
        v[i] = energies[i];
    }
    const double mean = de_tree_sum(v) / S;
    std::fill(v.begin(), v.end(), 0.0);
    for (int i = 0; i < S; ++i) { const double d = energies[i] - mean; v[i] = d * d; }
    const double sd = std::sqrt(de_tree_sum(v) / S);
    int best = 0;
    for (int i = 1; i < S; ++i) if (energies[i] < energies[best]) best = i;              // ties: the lowest index
    int64_t stop = 0;
    if (g > 0 && (g & 1) == 0) {
        if (std::isfinite(mean) && sd == sd && sd <= tol * std::fabs(mean)) stop |= HM_DE_STOP_CONVERGED;
        if (energies[best] < energy_limit) stop |= HM_DE_STOP_ENERGY;
    }
    if (g >= max_generations) stop |= HM_DE_STOP_MAX;
    auto bits = [](double d) { int64_t q; std::memcpy(&q, &d, 8); return q; };
    status[HM_DE_BEST_INDEX] = best;
    status[HM_DE_BEST_ENERGY] = bits(energies[best]);
    status[HM_DE_MEAN] = bits(mean);
    status[HM_DE_STD] = bits(sd);
    status[HM_DE_EVALUATIONS] += S;
    status[HM_DE_STOP] = stop;
    status[HM_DE_GENERATION] = g + 1;
}

size_t hm_de_workspace_bytes(int64_t, int, int) { return 0; }
int hm_de_generation(double* population, double* energies, double* trial, double* trial_energies, double* icrf, uint8_t* valid,
                     int64_t* status, const double* mean_icrf, const double* pca, const double* lower_limits,
                     const double* upper_limits, const uint8_t* dn, const double* std_, const double* exposures, int64_t n_pixels,
                     int n_frames, int lower, int upper, int pop_size, int n_params, int64_t seed, int64_t max_generations,
                     double mutation_lo, double mutation_hi, double recombination, double tol, double energy_limit, void*, void*) {
    const int rc0 = hm_rules::check_de_generation(1, population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca,
                                                  lower_limits, upper_limits, dn, exposures, n_pixels, n_frames, lower, upper, pop_size,
                                                  n_params, max_generations, mutation_lo, mutation_hi, recombination, tol, energy_limit);
    if (rc0 != HM_OK) return rc0;
    if (status[HM_DE_STOP] != 0) return HM_OK;                            // this build's own (status is host memory here): after the stop flag a generation is a no-op
    const int S = pop_size, P = n_params;
    const int64_t g = status[HM_DE_GENERATION];
    const uint64_t key = mix64(static_cast<uint64_t>(seed) ^ mix64(static_cast<uint64_t>(g)));
    const double F = mutation_lo + (mutation_hi - mutation_lo) * de_uniform(key, S, 0);
    const int b = std::min(std::max(static_cast<int>(status[HM_DE_BEST_INDEX]), 0), S - 1);
    for (int i = 0; i < S; ++i) {
        double x[HM_DE_MAX_PARAMS];
        const double* ui = population + static_cast<int64_t>(i) * P;
        double* tr = trial + static_cast<int64_t>(i) * P;
        const int pick = std::min(static_cast<int>(std::floor(de_uniform(key, i, 0) * (S - 1))), S - 2);
        const int r0 = pick + (pick >= i);
        int c = std::min(static_cast<int>(std::floor(de_uniform(key, i, 1) * (S - 2))), S - 3);
        const int lo2 = std::min(i, r0), hi2 = std::max(i, r0);
        c += (c >= lo2);
        c += (c >= hi2);
        const int r1 = c;
        const int fill = static_cast<int>(std::floor(de_uniform(key, i, 2) * P));
        for (int j = 0; j < P; ++j) {
            double v = ui[j];
            if (g > 0 && (de_uniform(key, i, 3 + j) < recombination || j == fill)) {
                const double ub = population[static_cast<int64_t>(b) * P + j], u0 = population[static_cast<int64_t>(r0) * P + j],
                             u1 = population[static_cast<int64_t>(r1) * P + j];
                v = ui[j] + F * (((ub - ui[j]) + u0) - u1);
                if (!(v >= 0.0 && v <= 1.0)) v = de_uniform(key, i, 3 + P + j);          // SciPy's _ensure_constraint
            }
            tr[j] = v;
            x[j] = lower_limits[j] + v * (upper_limits[j] - lower_limits[j]);
        }
        double* row = icrf + static_cast<int64_t>(i) * 256;
        for (int d = 0; d < 256; ++d) {
            double acc = 0.0;
            for (int j = 0; j < P; ++j) acc += pca[d * P + j] * x[j];
            row[d] = mean_icrf[d] + acc;
        }
        const double shift = 1.0 - row[255];
        for (int d = 0; d < 256; ++d) row[d] += shift;                                   // :166
        row[0] = 0.0;                                                                    // :167
        bool ok = true;
        for (int d = 0; d < 256; ++d)
            if (row[d] > 1.0 || row[d] < 0.0 || (d > 0 && !(row[d] > row[d - 1]))) ok = false;   // :173-179
        valid[i] = ok;
    }
    const int rc = hm_linearity_energy(dn, std_, exposures, icrf, valid, S, lower, upper, 1, n_pixels, n_frames, nullptr,
                                       trial_energies, nullptr, nullptr);
    if (rc != HM_OK) return rc;
    de_select_host(population, energies, trial, trial_energies, status, S, P, g, max_generations, tol, energy_limit);
    return HM_OK;
}

// ... on a uint16 stack of 9 to 16 bits, rows of R = 2^bit_depth entries (csrc/hm_de_u16.hip with host pointers): the trial component
// text the device kernels include, the row walk serially, hm_linearity_energy_u16 above, the selection of hm_de_generation
int hm_de_generation_u16(double* population, double* energies, double* trial, double* trial_energies, double* icrf, uint8_t* valid,
                         int64_t* status, const double* mean_icrf, const double* pca, const double* lower_limits,
                         const double* upper_limits, const uint16_t* dn, const double* std_, const double* exposures, int64_t n_pixels,
                         int n_frames, int lower, int upper, int pop_size, int n_params, int64_t seed, int64_t max_generations,
                         double mutation_lo, double mutation_hi, double recombination, double tol, double energy_limit, int bit_depth,
                         int variant, void*, void*) {
    const int rc0 = hm_rules::check_de_generation_u16(population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca,
                                                      lower_limits, upper_limits, dn, exposures, n_pixels, n_frames, lower, upper, pop_size,
                                                      n_params, max_generations, mutation_lo, mutation_hi, recombination, tol, energy_limit,
                                                      bit_depth, variant);
    if (rc0 != HM_OK) return rc0;
    if (status[HM_DE_STOP] != 0) return HM_OK;                            // this build's own, as in hm_de_generation
    using std::floor;
    using std::max;
    using std::min;
    const DeK a = de_args(population, energies, trial, trial_energies, icrf, valid, status, mean_icrf, pca, lower_limits, upper_limits,
                          pop_size, n_params, seed, max_generations, mutation_lo, mutation_hi, recombination, tol, energy_limit);
    const int S = pop_size, P = n_params, R = 1 << bit_depth;
    const int64_t g = status[HM_DE_GENERATION];
    for (int i = 0; i < S; ++i) {
        double x[HM_DE_MAX_PARAMS];
        for (int lane = 0; lane < P; ++lane) {
#include "../csrc/hm_de_trial_component_body.h"
        }
        double* row = icrf + static_cast<int64_t>(i) * R;
        for (int d = 0; d < R; ++d) {
            double acc = 0.0;
            for (int j = 0; j < P; ++j) acc += pca[d * P + j] * x[j];
            row[d] = mean_icrf[d] + acc;
        }
        const double shift = 1.0 - row[R - 1];
        for (int d = 0; d < R; ++d) row[d] += shift;                                     // :166
        row[0] = 0.0;                                                                    // :167
        bool ok = true;
        for (int d = 0; d < R; ++d)
            if (row[d] > 1.0 || row[d] < 0.0 || (d > 0 && !(row[d] > row[d - 1]))) ok = false;   // :173-179
        valid[i] = ok;
    }
    const int rc = hm_linearity_energy_u16(dn, std_, exposures, icrf, valid, S, lower, upper, 1, n_pixels, n_frames, bit_depth, variant, nullptr,
                                           trial_energies, nullptr, nullptr);
    if (rc != HM_OK) return rc;
    de_select_host(population, energies, trial, trial_energies, status, S, P, g, max_generations, tol, energy_limit);
    return HM_OK;
}

// n_problems problems of one shape per call (hdrmerge.h): on the host a batch IS its problems one after another, each through
// hm_de_generation above on its slices of the (K, ...) state - which returns at once for a problem whose stop flag is set
size_t hm_de_batch_workspace_bytes(int64_t, int, int, int) { return 0; }
int hm_de_generation_batch(int n_problems, double* population, double* energies, double* trial, double* trial_energies, double* icrf,
                           uint8_t* valid, int64_t* status, const double* mean_icrf, const double* pca, const double* lower_limits,
                           const double* upper_limits, const uint8_t* const* dn, const double* const* std_, const int64_t* seeds,
                           const double* exposures, int64_t n_pixels, int n_frames, int lower, int upper, int pop_size, int n_params,
                           int64_t max_generations, double mutation_lo, double mutation_hi, double recombination, double tol,
                           double energy_limit, void*, void*) {
    const int rc0 = hm_rules::check_de_generation_batch(n_problems, population, energies, trial, trial_energies, icrf, valid, status, mean_icrf,
                                                        pca, lower_limits, upper_limits, dn, std_, seeds, exposures, n_pixels, n_frames, lower,
                                                        upper, pop_size, n_params, max_generations, mutation_lo, mutation_hi, recombination,
                                                        tol, energy_limit);
    if (rc0 != HM_OK) return rc0;
    const int64_t S = pop_size, P = n_params;
    for (int64_t k = 0; k < n_problems; ++k) {
        const int rc = hm_de_generation(population + k * S * P, energies + k * S, trial + k * S * P, trial_energies + k * S,
                                        icrf + k * S * 256, valid + k * S, status + k * HM_DE_STATUS_WORDS, mean_icrf + k * 256,
                                        pca + k * 256 * P, lower_limits, upper_limits, dn[k], std_ ? std_[k] : nullptr, exposures,
                                        n_pixels, n_frames, lower, upper, pop_size, n_params, seeds[k], max_generations, mutation_lo,
                                        mutation_hi, recombination, tol, energy_limit, nullptr, nullptr);
        if (rc != HM_OK) return rc;
    }
    return HM_OK;
}

// ... and of uint16 stacks of one depth: each problem through hm_de_generation_u16 on its slices, rows of R = 2^bit_depth entries (a
// stopped problem is skipped there: it returns at once)
int hm_de_generation_u16_batch(int n_problems, double* population, double* energies, double* trial, double* trial_energies, double* icrf,
                               uint8_t* valid, int64_t* status, const double* mean_icrf, const double* pca, const double* lower_limits,
                               const double* upper_limits, const uint16_t* const* dn, const double* const* std_, const int64_t* seeds,
                               const double* exposures, int64_t n_pixels, int n_frames, int lower, int upper, int pop_size, int n_params,
                               int64_t max_generations, double mutation_lo, double mutation_hi, double recombination, double tol,
                               double energy_limit, int bit_depth, int variant, void*, void*) {
    const int rc0 = hm_rules::check_de_generation_u16_batch(n_problems, population, energies, trial, trial_energies, icrf, valid, status,
                                                            mean_icrf, pca, lower_limits, upper_limits, dn, std_, seeds, exposures, n_pixels,
                                                            n_frames, lower, upper, pop_size, n_params, max_generations, mutation_lo,
                                                            mutation_hi, recombination, tol, energy_limit, bit_depth, variant);
    if (rc0 != HM_OK) return rc0;
    const int64_t S = pop_size, P = n_params, R = int64_t{1} << bit_depth;
    for (int64_t k = 0; k < n_problems; ++k) {
        const int rc = hm_de_generation_u16(population + k * S * P, energies + k * S, trial + k * S * P, trial_energies + k * S,
                                            icrf + k * S * R, valid + k * S, status + k * HM_DE_STATUS_WORDS, mean_icrf + k * R,
                                            pca + k * R * P, lower_limits, upper_limits, dn[k], std_ ? std_[k] : nullptr, exposures,
                                            n_pixels, n_frames, lower, upper, pop_size, n_params, seeds[k], max_generations, mutation_lo,
                                            mutation_hi, recombination, tol, energy_limit, bit_depth, variant, nullptr, nullptr);
        if (rc != HM_OK) return rc;
    }
    return HM_OK;
}

/* ------------------------------------------------------------------------------------------
 * hm_tiff_decode_strips on the host: the same argument checks, status words and frame as the device entry point of
 * csrc/hm_tiff_device.hip, with HOST pointers - the decoder body both builds share (csrc/hm_tiff_lzw_body.h) with a serial emitter,
 * one strip per OpenMP iteration. It exists so that the host build carries the whole ABI; tiff_io.imread does not go through it.
 * ------------------------------------------------------------------------------------------ */
struct TiffSerialEmit {
    uint8_t* out;
    void literal(int64_t op, uint8_t b) { out[op] = b; }
    void copy(int64_t op, uint32_t from, uint32_t n, uint32_t period) {
        for (uint32_t k = 0; k < n; ++k) out[op + k] = out[from + (k < period ? k : k - period)];
    }
};

size_t hm_tiff_decode_workspace_bytes(int n_strips, int64_t strip_bytes, int compression) {
    return hm_rules::tiff_decode_workspace_bytes(n_strips, strip_bytes, compression);
}

int hm_tiff_decode_strips(const uint8_t* file, int64_t file_len, const int64_t* strip_offsets, const int64_t* strip_counts, int n_strips,
                          int compression, int predictor, int rows_per_strip, int height, int width, int samples, int bytes_per_sample,
                          int color_mode, void* dst_, int64_t* strip_status, void* workspace, void* /*stream*/) {
    static_assert(int(hm_lzw::kEinval) == int(HM_EINVAL) && int(hm_lzw::kEshape) == int(HM_ESHAPE), "hm_tiff_lzw_body.h repeats two codes of hdrmerge.h");
    hm_rules::TiffDecodeGeom geom;
    const int rc = hm_rules::check_tiff_decode(file, file_len, strip_offsets, strip_counts, n_strips, compression, predictor, rows_per_strip,
                                               height, width, samples, bytes_per_sample, color_mode, dst_, strip_status, workspace, geom);
    if (rc != HM_OK) return rc;
    const int rps = geom.rps;
    const int64_t row_bytes = geom.row_bytes, strip_bytes = geom.strip_bytes;
    const int spp = samples, bps = bytes_per_sample, ospp = color_mode == 1 ? 3 : samples;
    const int64_t out_row_bytes = static_cast<int64_t>(width) * ospp * bps;
    uint8_t* dst = static_cast<uint8_t*>(dst_);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
#pragma omp parallel for schedule(dynamic)
    for (int s = 0; s < n_strips; ++s) {
        const int64_t o = strip_offsets[s], c = strip_counts[s];
        const int rows = std::min(rps, height - s * rps);
        const int64_t want = rows * row_bytes;
        if (!(o >= 0 && c >= 0 && o <= file_len && c <= file_len - o)) { strip_status[s] = HM_EINVAL; continue; }
        const uint8_t* in = file + o;
        int64_t st = std::min(c, want);
        if (compression == 5) {
            std::vector<hm_lzw::Table> table(1);
            TiffSerialEmit emit{ws + s * strip_bytes};
            st = hm_lzw::decode(file + o, c, want, table[0], emit);
            in = emit.out;
        }
        strip_status[s] = st;
        if (st <= 0) continue;
        for (int r = 0; r < rows; ++r) {
            const int64_t avail = std::min(st, want) - r * row_bytes;
            if (avail <= 0) break;
            const int npx = avail >= row_bytes ? width : static_cast<int>(avail / (spp * bps));
            const uint8_t* row_in = in + r * row_bytes;
            uint8_t* out = dst + (static_cast<int64_t>(s) * rps + r) * out_row_bytes;
            uint8_t run[4] = {0, 0, 0, 0};
            for (int px = 0; px < npx; ++px)
                for (int ch = 0; ch < ospp; ++ch) {
                    const int sc = spp >= 3 ? (ch < 3 ? 2 - ch : ch) : 0;
                    if (bps == 8) { memcpy(out + (static_cast<int64_t>(px) * ospp + ch) * 8, row_in + (static_cast<int64_t>(px) * spp + sc) * 8, 8); continue; }
                    uint8_t v = row_in[static_cast<int64_t>(px) * spp + sc];
                    if (predictor == 2) {
                        if (spp == 1 && ch > 0) v = run[0];                      // grey replicated: the sum was advanced by channel 0
                        else v = run[sc] = static_cast<uint8_t>(run[sc] + v);
                    }
                    out[static_cast<int64_t>(px) * ospp + ch] = v;
                }
        }
    }
    return HM_OK;
}

/* ------------------------------------------------------------------------------------------
 * hm_tiff_decode_strips_wide on the host: 2-, 4- and 8-byte samples of either byte order. The same rule function, status words and
 * frame as the device entry point; the row is the text both builds share (csrc/hm_tiff_wide_body.h) with one pixel per step, its
 * loads of samples at odd offsets go through memcpy. One strip per OpenMP iteration, as above.
 * ------------------------------------------------------------------------------------------ */
struct TiffSerialLanes {
    int width() const { return 1; }
    int lane() const { return 0; }
    uint32_t scan_add(uint32_t x) const { return x; }
    uint32_t last(uint32_t x) const { return x; }
};

int hm_tiff_decode_strips_wide(const uint8_t* file, int64_t file_len, const int64_t* strip_offsets, const int64_t* strip_counts,
                               int n_strips, int compression, int predictor, int rows_per_strip, int height, int width, int samples,
                               int bytes_per_sample, int big_endian, int color_mode, void* dst_, int64_t* strip_status,
                               void* workspace, void* /*stream*/) {
    hm_rules::TiffDecodeGeom geom;
    const int rc = hm_rules::check_tiff_decode_wide(file, file_len, strip_offsets, strip_counts, n_strips, compression, predictor,
                                                    rows_per_strip, height, width, samples, bytes_per_sample, big_endian, color_mode, dst_,
                                                    strip_status, workspace, geom);
    if (rc != HM_OK) return rc;
    const int rps = geom.rps;
    const int64_t row_bytes = geom.row_bytes, strip_bytes = geom.strip_bytes;
    const int spp = samples, bps = bytes_per_sample;
    const int64_t out_row_bytes = static_cast<int64_t>(width) * (color_mode == 1 ? 3 : spp * bps);
    uint8_t* dst = static_cast<uint8_t*>(dst_);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
#pragma omp parallel for schedule(dynamic)
    for (int s = 0; s < n_strips; ++s) {
        const int64_t o = strip_offsets[s], c = strip_counts[s];
        const int rows = std::min(rps, height - s * rps);
        const int64_t want = rows * row_bytes;
        if (!(o >= 0 && c >= 0 && o <= file_len && c <= file_len - o)) { strip_status[s] = HM_EINVAL; continue; }
        const uint8_t* in = file + o;
        int64_t st = std::min(c, want);
        if (compression == 5) {
            std::vector<hm_lzw::Table> table(1);
            TiffSerialEmit emit{ws + s * strip_bytes};
            st = hm_lzw::decode(file + o, c, want, table[0], emit);
            in = emit.out;
        }
        strip_status[s] = st;
        if (st <= 0) continue;
        TiffSerialLanes lanes;
        for (int r = 0; r < rows; ++r) {
            const int64_t avail = std::min(st, want) - r * row_bytes;
            if (avail <= 0) break;
            const int npx = avail >= row_bytes ? width : static_cast<int>(avail / (spp * bps));
            const uint8_t* row_in = in + r * row_bytes;
            uint8_t* out = dst + (static_cast<int64_t>(s) * rps + r) * out_row_bytes;
            if (bps == 2) hm_tiff_wide::finish_row<2>(row_in, npx, spp, big_endian != 0, predictor, color_mode, out, lanes);
            else if (bps == 4) hm_tiff_wide::finish_row<4>(row_in, npx, spp, big_endian != 0, predictor, color_mode, out, lanes);
            else hm_tiff_wide::finish_row<8>(row_in, npx, spp, big_endian != 0, predictor, color_mode, out, lanes);
        }
    }
    return HM_OK;
}

/* ------------------------------------------------------------------------------------------
 * hm_tiff_encode_strips on the host: the same argument checks, payload layout and bytes as the device entry point of
 * csrc/hm_tiff_encode.hip, with HOST pointers - the encoder body both builds share (csrc/hm_tiff_lzw_enc_body.h) with its serial ops,
 * one strip per OpenMP iteration. tiff_io.imwrite(compression=5) writes through it, and the GPU tests compare the device call with it.
 * ------------------------------------------------------------------------------------------ */
// the offsets from the counts (each rounded up to 16) and the streams moved from their slots behind the packed strips into the payload
static void tiff_compact_strips(uint8_t* payload, const uint8_t* streams, int64_t out_pitch, int n_strips, int64_t* offsets,
                                const int64_t* counts) {
    int64_t total = 0;
    for (int s = 0; s < n_strips; ++s) {
        offsets[s] = total;
        total += counts[s] > 0 ? hm_rules::round16(counts[s]) : 0;
    }
    offsets[n_strips] = total;
#pragma omp parallel for schedule(dynamic)
    for (int s = 0; s < n_strips; ++s) {
        if (counts[s] <= 0) continue;
        uint8_t* out = payload + offsets[s];
        memcpy(out, streams + s * out_pitch, static_cast<size_t>(counts[s]));
        memset(out + counts[s], 0, static_cast<size_t>(hm_rules::round16(counts[s]) - counts[s]));       // the gap: zeros, never stale memory
    }
}

int64_t hm_tiff_encode_bound(int64_t strip_bytes) { return hm_rules::tiff_encode_bound(strip_bytes); }

size_t hm_tiff_encode_workspace_bytes(int n_strips, int64_t strip_bytes, int compression) {
    return hm_rules::tiff_encode_workspace_bytes(n_strips, strip_bytes, compression);
}

size_t hm_tiff_encode_payload_bytes(int n_strips, int64_t strip_bytes, int compression) {
    return hm_rules::tiff_encode_payload_bytes(n_strips, strip_bytes, compression);
}

int hm_tiff_encode_strips(const void* src_, int src_kind, double divisor, int height, int width, int samples, int rows_per_strip,
                          int compression, int predictor, void* payload_, int64_t payload_cap, void* strip_offsets, void* strip_counts,
                          void* workspace, void* /*stream*/) {
    static_assert(int(hm_lzw_enc::kEshape) == int(HM_ESHAPE), "hm_tiff_lzw_enc_body.h repeats a code of hdrmerge.h");
    hm_rules::TiffEncodeGeom geom;
    const int rc = hm_rules::check_tiff_encode(src_, src_kind, divisor, height, width, samples, rows_per_strip, compression, predictor, payload_,
                                               payload_cap, strip_offsets, strip_counts, workspace, geom);
    if (rc != HM_OK) return rc;
    const int rps = geom.rps, n_strips = geom.n_strips;
    const int64_t row_bytes = geom.row_bytes, strip_bytes = geom.strip_bytes;
    const uint8_t* src = static_cast<const uint8_t*>(src_);
    uint8_t* payload = static_cast<uint8_t*>(payload_);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    int64_t* offsets = static_cast<int64_t*>(strip_offsets);
    int64_t* counts = static_cast<int64_t*>(strip_counts);
    const int spp = samples;
    const int64_t bound = geom.bound, in_pitch = geom.in_pitch, out_pitch = geom.out_pitch;
#pragma omp parallel for schedule(dynamic)
    for (int s = 0; s < n_strips; ++s) {
        const int rows = std::min(rps, height - s * rps);
        const int64_t len = rows * row_bytes;
        uint8_t* packed = compression == 1 ? payload + s * strip_bytes : ws + s * in_pitch;
        for (int r = 0; r < rows; ++r) {
            const int64_t in_row = (static_cast<int64_t>(s) * rps + r) * width * spp;          // in samples
            uint8_t* out = packed + r * row_bytes;
            for (int px = 0; px < width; ++px)
                for (int ch = 0; ch < spp; ++ch) {
                    const int64_t at = in_row + static_cast<int64_t>(px) * spp + (spp >= 3 ? (ch < 3 ? 2 - ch : ch) : 0);
                    if (src_kind == 1) { memcpy(out + (static_cast<int64_t>(px) * spp + ch) * 8, src + at * 8, 8); continue; }
                    auto sample = [&](int64_t k) {
                        if (src_kind == 0) return src[k];
                        double v;
                        memcpy(&v, src + k * 8, 8);
                        return hm_lzw_enc::quantize_u8(v, divisor);
                    };
                    const uint8_t v = sample(at), left = predictor == 2 && px > 0 ? sample(at - spp) : uint8_t{0};
                    out[static_cast<int64_t>(px) * spp + ch] = static_cast<uint8_t>(v - left);
                }
        }
        if (compression == 1) {
            offsets[s] = s * strip_bytes;
            counts[s] = len;
        } else {
            std::vector<hm_lzw_enc::Dict> dict(1);
            hm_lzw_enc::SerialOps ops;
            counts[s] = hm_lzw_enc::encode(packed, len, ws + n_strips * in_pitch + s * out_pitch, bound, dict[0], ops);
        }
    }
    if (compression == 1) {
        offsets[n_strips] = static_cast<int64_t>(height) * row_bytes;
        return HM_OK;
    }
    tiff_compact_strips(payload, ws + n_strips * in_pitch, out_pitch, n_strips, offsets, counts);
    return HM_OK;
}

/* ------------------------------------------------------------------------------------------
 * hm_tiff_encode_strips_wide on the host: 2- and 4-byte stored samples. The same rule function, payload layout and bytes as the device
 * entry point; the row is the text both builds share (csrc/hm_tiff_wide_enc_body.h) with one sample per step, the LZW stage and the
 * compaction are those of hm_tiff_encode_strips above. One strip per OpenMP iteration. tiff_io.imwrite(wide_samples=True) writes
 * through it.
 * ------------------------------------------------------------------------------------------ */
struct TiffEncSerialLanes {
    int width() const { return 1; }
    int lane() const { return 0; }
};

int hm_tiff_encode_strips_wide(const void* src_, int src_kind, double divisor, int max_dn, int height, int width, int samples,
                               int rows_per_strip, int compression, int predictor, void* payload_, int64_t payload_cap,
                               void* strip_offsets, void* strip_counts, void* workspace, void* /*stream*/) {
    hm_rules::TiffEncodeGeom geom;
    const int rc = hm_rules::check_tiff_encode_wide(src_, src_kind, divisor, max_dn, height, width, samples, rows_per_strip, compression,
                                                    predictor, payload_, payload_cap, strip_offsets, strip_counts, workspace, geom);
    if (rc != HM_OK) return rc;
    const int rps = geom.rps, n_strips = geom.n_strips;
    const int64_t row_bytes = geom.row_bytes, strip_bytes = geom.strip_bytes;
    const uint8_t* src = static_cast<const uint8_t*>(src_);
    uint8_t* payload = static_cast<uint8_t*>(payload_);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    int64_t* offsets = static_cast<int64_t*>(strip_offsets);
    int64_t* counts = static_cast<int64_t*>(strip_counts);
    const int in_bps = src_kind == HM_TIFF_SRC_U16 ? 2 : (src_kind == HM_TIFF_SRC_F32 ? 4 : 8);
    const int64_t in_row_bytes = static_cast<int64_t>(width) * samples * in_bps;
    const int64_t bound = geom.bound, in_pitch = geom.in_pitch, out_pitch = geom.out_pitch;
#pragma omp parallel for schedule(dynamic)
    for (int s = 0; s < n_strips; ++s) {
        const int rows = std::min(rps, height - s * rps);
        const int64_t len = rows * row_bytes;
        uint8_t* packed = compression == 1 ? payload + s * strip_bytes : ws + s * in_pitch;
        TiffEncSerialLanes lanes;
        for (int r = 0; r < rows; ++r) {
            const uint8_t* in = src + (static_cast<int64_t>(s) * rps + r) * in_row_bytes;
            uint8_t* out = packed + r * row_bytes;
            if (geom.out_bps == 2) hm_tiff_wide_enc::pack_row<2>(in, src_kind, divisor, max_dn, width, samples, predictor, out, lanes);
            else hm_tiff_wide_enc::pack_row<4>(in, src_kind, divisor, max_dn, width, samples, predictor, out, lanes);
        }
        if (compression == 1) {
            offsets[s] = s * strip_bytes;
            counts[s] = len;
        } else {
            std::vector<hm_lzw_enc::Dict> dict(1);
            hm_lzw_enc::SerialOps ops;
            counts[s] = hm_lzw_enc::encode(packed, len, ws + n_strips * in_pitch + s * out_pitch, bound, dict[0], ops);
        }
    }
    if (compression == 1) {
        offsets[n_strips] = static_cast<int64_t>(height) * row_bytes;
        return HM_OK;
    }
    tiff_compact_strips(payload, ws + n_strips * in_pitch, out_pitch, n_strips, offsets, counts);
    return HM_OK;
}

}  // extern "C"
