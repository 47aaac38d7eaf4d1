// hm_tiff_rules.h - the argument rules and size functions of the TIFF strip entries (hm_tiff_decode_strips, hm_tiff_decode_strips_wide,
// hm_tiff_encode_strips, hm_tiff_encode_strips_wide and their _workspace_bytes / _bound / _payload_bytes), written once for both builds of the ABI in the manner of hm_merge_rules.h: the device build
// (hm_tiff_device.hip, hm_tiff_encode.hip) and the host build (csrc_host/hm_host.cpp) include this file and hold no argument test of
// their own for these entries. Plain C++17 on hdrmerge.h, the encoder body's size bound and the standard headers: no HIP type.
//
// Every status a call can be refused with is here, in the order hdrmerge.h gives them: an earlier rule wins over a later one broken in
// the same call. A check also returns the geometry both builds derive from a valid call. There is no difference between the builds: both
// need the workspace for Compression 5, and both refuse the same pointers' alignment.
#pragma once
#include "hdrmerge.h"
#include "hm_tiff_lzw_enc_body.h"
#include <cstddef>
#include <cstdint>

namespace hm_rules {

// the largest strip (rows per strip x stored row bytes) of each entry: the decoder takes 2^31 bytes, the encoder one byte less
constexpr int64_t kTiffDecodeMaxStripBytes = int64_t{1} << 31;
constexpr int64_t kTiffEncodeMaxStripBytes = hm_lzw_enc::kMaxInput;       // 2^31 - 1

constexpr int64_t round16(int64_t x) { return (x + 15) & ~int64_t{15}; }   // (constexpr: callable from kernels as well)
inline bool tiff_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

struct TiffDecodeGeom {
    int rps;                                 // rows per strip, clamped to the height
    int64_t row_bytes;                       // of the stored layout
    int64_t strip_bytes;                     // rps * row_bytes: the pitch of the workspace
};

struct TiffEncodeGeom {
    int rps, n_strips;
    int out_bps;                             // bytes per stored sample: 1 or 8 (hm_tiff_encode_strips), 2 or 4 (_wide)
    int64_t row_bytes, strip_bytes;
    int64_t bound;                           // hm_lzw_enc::bound(strip_bytes)
    int64_t in_pitch, out_pitch;             // compression 5: round16(strip_bytes), round16(bound) - the workspace's two pitches
};

inline size_t tiff_decode_workspace_bytes(int n_strips, int64_t strip_bytes, int compression) {
    if (compression != 5 || n_strips < 1 || strip_bytes < 1 || strip_bytes > kTiffDecodeMaxStripBytes) return 0;
    return static_cast<size_t>(n_strips) * static_cast<size_t>(strip_bytes);
}

inline int check_tiff_decode(const uint8_t* file, int64_t file_len, const int64_t* strip_offsets, const int64_t* strip_counts, int n_strips,
                             int compression, int predictor, int rows_per_strip, int height, int width, int samples,
                             int bytes_per_sample, int color_mode, const void* dst, const int64_t* strip_status, const void* workspace,
                             TiffDecodeGeom& g) {
    g = TiffDecodeGeom{};
    if (!file || !strip_offsets || !strip_counts || !dst || !strip_status || file_len < 0) return HM_EINVAL;
    if (n_strips < 1 || rows_per_strip < 1 || height < 1 || width < 1) return HM_EINVAL;
    if (predictor != 1 && predictor != 2) return HM_EINVAL;
    if (color_mode != 0 && color_mode != 1) return HM_EINVAL;
    if (compression != 1 && compression != 5) return HM_EUNSUPPORTED;
    if (samples != 1 && samples != 3 && samples != 4) return HM_EUNSUPPORTED;
    if (bytes_per_sample != 1 && bytes_per_sample != 8) return HM_EUNSUPPORTED;
    if (bytes_per_sample == 8 && (predictor == 2 || color_mode == 1)) return HM_EUNSUPPORTED;
    g.rps = rows_per_strip < height ? rows_per_strip : height;
    if (n_strips != (height - 1) / g.rps + 1) return HM_ESHAPE;                    // ceil(height / rps) without height + rps: no int overflow
    g.row_bytes = static_cast<int64_t>(width) * samples * bytes_per_sample;
    if (g.row_bytes > kTiffDecodeMaxStripBytes / g.rps) return HM_ESHAPE;
    g.strip_bytes = g.row_bytes * g.rps;
    if (compression == 5 && !workspace) return HM_EINVAL;
    return HM_OK;
}

// hm_tiff_decode_strips_wide: the same geometry for 2-, 4- and 8-byte samples of either byte order. 1-byte samples belong to the entry
// above; Predictor 2 and the 8-bit conversion (color_mode 1) exist for 2-byte samples only. In color_mode 0 dst holds samples and must
// be aligned to them; in color_mode 1 it holds bytes.
inline int check_tiff_decode_wide(const uint8_t* file, int64_t file_len, const int64_t* strip_offsets, const int64_t* strip_counts,
                                  int n_strips, int compression, int predictor, int rows_per_strip, int height, int width, int samples,
                                  int bytes_per_sample, int big_endian, int color_mode, const void* dst, const int64_t* strip_status,
                                  const void* workspace, TiffDecodeGeom& g) {
    g = TiffDecodeGeom{};
    if (!file || !strip_offsets || !strip_counts || !dst || !strip_status || file_len < 0) return HM_EINVAL;
    if (n_strips < 1 || rows_per_strip < 1 || height < 1 || width < 1) return HM_EINVAL;
    if (predictor != 1 && predictor != 2) return HM_EINVAL;
    if (color_mode != 0 && color_mode != 1) return HM_EINVAL;
    if (big_endian != 0 && big_endian != 1) return HM_EINVAL;
    if (compression == 5 && !workspace) return HM_EINVAL;
    if (compression != 1 && compression != 5) return HM_EUNSUPPORTED;
    if (samples != 1 && samples != 3 && samples != 4) return HM_EUNSUPPORTED;
    if (bytes_per_sample != 2 && bytes_per_sample != 4 && bytes_per_sample != 8) return HM_EUNSUPPORTED;
    if (bytes_per_sample != 2 && (predictor == 2 || color_mode == 1)) return HM_EUNSUPPORTED;
    g.rps = rows_per_strip < height ? rows_per_strip : height;
    if (n_strips != (height - 1) / g.rps + 1) return HM_ESHAPE;                    // as above
    g.row_bytes = static_cast<int64_t>(width) * samples * bytes_per_sample;
    if (g.row_bytes > kTiffDecodeMaxStripBytes / g.rps) return HM_ESHAPE;
    g.strip_bytes = g.row_bytes * g.rps;
    if (color_mode == 0 && !tiff_aligned(dst, static_cast<uintptr_t>(bytes_per_sample))) return HM_EALIGN;
    return HM_OK;
}

inline int64_t tiff_encode_bound(int64_t strip_bytes) {
    if (strip_bytes < 1) return HM_EINVAL;
    if (strip_bytes > kTiffEncodeMaxStripBytes) return HM_ESHAPE;
    return hm_lzw_enc::bound(strip_bytes);
}

inline size_t tiff_encode_workspace_bytes(int n_strips, int64_t strip_bytes, int compression) {
    if (compression != 5 || n_strips < 1 || strip_bytes < 1 || strip_bytes > kTiffEncodeMaxStripBytes) return 0;
    return static_cast<size_t>(n_strips) * static_cast<size_t>(round16(strip_bytes) + round16(hm_lzw_enc::bound(strip_bytes)));
}

inline size_t tiff_encode_payload_bytes(int n_strips, int64_t strip_bytes, int compression) {
    if ((compression != 1 && compression != 5) || n_strips < 1 || strip_bytes < 1 || strip_bytes > kTiffEncodeMaxStripBytes) return 0;
    if (compression == 1) return static_cast<size_t>(n_strips) * static_cast<size_t>(strip_bytes);
    return static_cast<size_t>(n_strips) * static_cast<size_t>(round16(hm_lzw_enc::bound(strip_bytes)));
}

inline int check_tiff_encode(const void* src, int src_kind, double divisor, int height, int width, int samples, int rows_per_strip,
                             int compression, int predictor, const void* payload, int64_t payload_cap, const void* strip_offsets,
                             const void* strip_counts, const void* workspace, TiffEncodeGeom& g) {
    g = TiffEncodeGeom{};
    if (!src || !payload || !strip_offsets || !strip_counts) return HM_EINVAL;
    if (height < 1 || width < 1 || rows_per_strip < 1) return HM_EINVAL;
    if (predictor != 1 && predictor != 2) return HM_EINVAL;
    if (compression != 1 && compression != 5) return HM_EUNSUPPORTED;
    if (samples != 1 && samples != 3 && samples != 4) return HM_EUNSUPPORTED;
    if (src_kind < 0 || src_kind > 2) return HM_EUNSUPPORTED;
    if (src_kind == 2 && !(divisor > 0.0 && divisor <= 1.7976931348623157e308)) return HM_EINVAL;      // finite and positive
    g.out_bps = src_kind == 1 ? 8 : 1;
    if (g.out_bps == 8 && predictor == 2) return HM_EUNSUPPORTED;
    g.rps = rows_per_strip < height ? rows_per_strip : height;
    g.n_strips = (height - 1) / g.rps + 1;                                         // ceil(height / rps), as above
    g.row_bytes = static_cast<int64_t>(width) * samples * g.out_bps;
    if (g.row_bytes > kTiffEncodeMaxStripBytes / g.rps) return HM_ESHAPE;
    g.strip_bytes = g.row_bytes * g.rps;
    g.bound = hm_lzw_enc::bound(g.strip_bytes);
    g.in_pitch = round16(g.strip_bytes);
    g.out_pitch = round16(g.bound);
    if (compression == 5 && !workspace) return HM_EINVAL;
    if (payload_cap < 0 || static_cast<uint64_t>(payload_cap) < tiff_encode_payload_bytes(g.n_strips, g.strip_bytes, compression)) return HM_ESHAPE;
    if (!tiff_aligned(payload, 16) || !tiff_aligned(strip_offsets, 8) || !tiff_aligned(strip_counts, 8) ||
        !tiff_aligned(src, src_kind == 0 ? 1 : 8) || (compression == 5 && !tiff_aligned(workspace, 16)))
        return HM_EALIGN;
    return HM_OK;
}

// hm_tiff_encode_strips_wide: the same geometry for 2- and 4-byte stored samples. Source kinds 0 uint16, 1 float32, 2 float64 narrowed to
// float32, 3 float64 quantised to uint16 (divisor and max_dn are read for kind 3 only); Predictor 2 exists for uint16 output only. The
// order of the statuses: HM_EINVAL (pointers, sizes, predictor; then kind 3's divisor and max_dn and the workspace of Compression 5),
// HM_EUNSUPPORTED (compression, samples, kind, Predictor 2 with float32 output), HM_ESHAPE (strip size, payload_cap), HM_EALIGN.
inline int check_tiff_encode_wide(const void* src, int src_kind, double divisor, int max_dn, int height, int width, int samples,
                                  int rows_per_strip, int compression, int predictor, const void* payload, int64_t payload_cap,
                                  const void* strip_offsets, const void* strip_counts, const void* workspace, TiffEncodeGeom& g) {
    g = TiffEncodeGeom{};
    if (!src || !payload || !strip_offsets || !strip_counts) return HM_EINVAL;
    if (height < 1 || width < 1 || rows_per_strip < 1) return HM_EINVAL;
    if (predictor != 1 && predictor != 2) return HM_EINVAL;
    if (src_kind == HM_TIFF_SRC_F64_AS_U16 && !(divisor > 0.0 && divisor <= 1.7976931348623157e308)) return HM_EINVAL;   // finite and positive
    if (src_kind == HM_TIFF_SRC_F64_AS_U16 && (max_dn < 1 || max_dn > 65535)) return HM_EINVAL;
    if (compression == 5 && !workspace) return HM_EINVAL;
    if (compression != 1 && compression != 5) return HM_EUNSUPPORTED;
    if (samples != 1 && samples != 3 && samples != 4) return HM_EUNSUPPORTED;
    if (src_kind < HM_TIFF_SRC_U16 || src_kind > HM_TIFF_SRC_F64_AS_U16) return HM_EUNSUPPORTED;
    g.out_bps = (src_kind == HM_TIFF_SRC_U16 || src_kind == HM_TIFF_SRC_F64_AS_U16) ? 2 : 4;
    if (g.out_bps == 4 && predictor == 2) return HM_EUNSUPPORTED;
    g.rps = rows_per_strip < height ? rows_per_strip : height;
    g.n_strips = (height - 1) / g.rps + 1;                                         // ceil(height / rps), as above
    g.row_bytes = static_cast<int64_t>(width) * samples * g.out_bps;
    if (g.row_bytes > kTiffEncodeMaxStripBytes / g.rps) return HM_ESHAPE;
    g.strip_bytes = g.row_bytes * g.rps;
    g.bound = hm_lzw_enc::bound(g.strip_bytes);
    g.in_pitch = round16(g.strip_bytes);
    g.out_pitch = round16(g.bound);
    if (payload_cap < 0 || static_cast<uint64_t>(payload_cap) < tiff_encode_payload_bytes(g.n_strips, g.strip_bytes, compression)) return HM_ESHAPE;
    const uintptr_t src_sample = src_kind == HM_TIFF_SRC_U16 ? 2 : (src_kind == HM_TIFF_SRC_F32 ? 4 : 8);
    if (!tiff_aligned(payload, 16) || !tiff_aligned(strip_offsets, 8) || !tiff_aligned(strip_counts, 8) || !tiff_aligned(src, src_sample) ||
        (compression == 5 && !tiff_aligned(workspace, 16)))
        return HM_EALIGN;
    return HM_OK;
}

}  // namespace hm_rules
