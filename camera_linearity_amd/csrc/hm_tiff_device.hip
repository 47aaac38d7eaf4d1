// hm_tiff_device.hip - TIFF strips decoded on the device: hm_tiff_decode_strips, hm_tiff_decode_strips_wide (include/hdrmerge.h). The neighbour of hm_tiff.hip
// (the host decoders, unchanged and still the default path of tiff_io.imread): the file's bytes are uploaded as they are, and two
// kernels turn them into the frame cv.imread would return.
//
//   lzw_strips_kernel   Compression 5. One strip per WAVE: the decoder state (bit accumulator, code width, next, old) is wave-uniform,
//                       every lane runs the same loop of hm_tiff_lzw_body.h, and only the copy of an emitted string is spread over the
//                       lanes. The string table - (position, length) into the output, 24 KiB - is the wave's own slice of LDS.
//                       Strips of at most kStageBytes are decoded into a second LDS slice (16 KiB) and written out once, coalesced;
//                       longer strips are decoded in place in the workspace (global memory), where every emission that reads waits for
//                       the stores before it.  LDS per wave 40 KiB (24 KiB in place): 2 waves per workgroup, 2 (3) workgroups per CU,
//                       so 4 (6) waves of the 32 a CU can hold - LDS is what bounds occupancy, and the loop is latency-bound (one
//                       dependent LDS round trip per code), not bandwidth-bound. Measured figures: DESIGN.md 4.4.5.
//   finish_rows_kernel  One row per wave, 64 pixels per step: undoes Predictor 2 (a wave-wide inclusive scan modulo 256 per sample with a
//                       carry between steps), swaps R and B at sample granularity, applies cv.imread's flag (IMREAD_COLOR: grey
//                       replicated, alpha dropped) and writes the final frame. Compression 1 reads the strips straight from the file
//                       bytes, so it is the only kernel of that path.
//   wide_rows_kernel    finish_rows_kernel's geometry for 2-, 4- and 8-byte samples of either byte order (hm_tiff_decode_strips_wide):
//                       the row itself is hm_tiff_wide_body.h, the text the host build runs serially, with the wave as its lanes -
//                       sample-wide loads and stores (byte loads only for a strip at an odd offset), the byte reversal, the scan
//                       modulo 65536 on the reversed values, the R/B swap and imread's >> 8. LZW is byte-oriented: lzw_strips_kernel
//                       serves both entries as it is.
//
// Safety: a strip's [offset, offset + count) is checked against file_len before anything of it is read; the decoder's bounds are those
// stated in hm_tiff_lzw_body.h; a strip that fails gets a negative status and its rows of dst are left untouched. No atomics, no
// allocation, no host synchronisation.
#include "hm_common.h"
#include "hm_tiff_lzw_body.h"
#include "hm_tiff_rules.h"
#include "hm_tiff_wide_body.h"

static_assert(int(hm_lzw::kEinval) == int(HM_EINVAL) && int(hm_lzw::kEshape) == int(HM_ESHAPE), "hm_tiff_lzw_body.h repeats two codes of hdrmerge.h");

namespace {

constexpr int kLzwWaves = 2;                 // waves (= strips) per workgroup of the decoder
constexpr int kStageBytes = 16 * 1024;       // strips up to this size are decoded in LDS (a 4096-wide RGB row is 12 KiB)

struct StripGeom {
    const uint8_t* file;
    int64_t file_len;
    const int64_t* offsets;
    const int64_t* counts;
    int n_strips;
    int rps;                                 // rows per strip, already clamped to the height
    int height;
    int width;
    int64_t row_bytes;                       // of the stored layout
    int64_t strip_bytes;                     // rps * row_bytes: the pitch of the workspace
    int64_t* status;
    uint8_t* workspace;
};

__device__ __forceinline__ bool strip_range_ok(int64_t o, int64_t c, int64_t file_len) {
    return o >= 0 && c >= 0 && o <= file_len && c <= file_len - o;
}

// the wave's emitter: `out` is the wave's slice of LDS or its strip of the workspace
struct WaveEmit {
    uint8_t* out;
    int lane;
    __device__ __forceinline__ void literal(int64_t op, uint8_t b) {
        if (lane == 0) out[op] = b;
    }
    __device__ __forceinline__ void copy(int64_t op, uint32_t from, uint32_t n, uint32_t period) {
        __threadfence_block();               // the source was written by other lanes of this wave: their stores complete before it is read
        for (uint32_t k = lane; k < n; k += hm::kWave) out[op + k] = out[from + (k < period ? k : k - period)];
    }
};

template <bool STAGE>
__global__ __launch_bounds__(kLzwWaves * hm::kWave) void lzw_strips_kernel(const StripGeom g) {
    __shared__ hm_lzw::Table tables[kLzwWaves];
    __shared__ uint8_t stage[STAGE ? kLzwWaves : 1][STAGE ? kStageBytes : 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.x * kLzwWaves + wave;
    if (s >= g.n_strips) return;
    const int64_t o = g.offsets[s], c = g.counts[s];
    if (!strip_range_ok(o, c, g.file_len)) {
        if (lane == 0) g.status[s] = HM_EINVAL;
        return;
    }
    const int rows_left = g.height - s * g.rps;
    const int64_t want = static_cast<int64_t>(rows_left < g.rps ? rows_left : g.rps) * g.row_bytes;     // <= strip_bytes (<= kStageBytes if STAGE)
    uint8_t* strip = g.workspace + static_cast<int64_t>(s) * g.strip_bytes;
    WaveEmit emit{STAGE ? stage[wave] : strip, lane};
    const int64_t r = hm_lzw::decode(g.file + o, c, want, tables[wave], emit);
    if (STAGE && r > 0) {
        __threadfence_block();
        for (int64_t k = lane; k < r; k += hm::kWave) strip[k] = stage[wave][k];
    }
    if (lane == 0) g.status[s] = r;
}

struct FinishGeom {
    StripGeom g;
    int compression, predictor, spp, bps, out_spp;
    uint8_t* dst;
};

__device__ __forceinline__ int src_channel(int c, int spp) { return spp >= 3 ? (c < 3 ? 2 - c : c) : 0; }

__global__ __launch_bounds__(256) void finish_rows_kernel(const FinishGeom f) {
    const StripGeom& g = f.g;
    const int lane = threadIdx.x & 63;
    const int spp = f.spp, ospp = f.out_spp;
    const int64_t out_row_bytes = static_cast<int64_t>(g.width) * ospp * f.bps;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); row < g.height; row += static_cast<int64_t>(gridDim.x) * 4) {
        const int s = static_cast<int>(row / g.rps);
        const int r = static_cast<int>(row - static_cast<int64_t>(s) * g.rps);
        const int rows_left = g.height - s * g.rps;
        const int64_t want = static_cast<int64_t>(rows_left < g.rps ? rows_left : g.rps) * g.row_bytes;
        const uint8_t* in;
        int64_t st;
        if (f.compression == 1) {
            const int64_t o = g.offsets[s], c = g.counts[s];
            st = strip_range_ok(o, c, g.file_len) ? (c < want ? c : want) : static_cast<int64_t>(HM_EINVAL);
            if (r == 0 && lane == 0) g.status[s] = st;
            in = g.file + o;
        } else {
            st = g.status[s];
            in = g.workspace + static_cast<int64_t>(s) * g.strip_bytes;
        }
        // a failed strip: nothing of it is read, its rows stay as they were. A short one (a stream that ends early) gives the whole pixels
        // it holds, like the host decoder's partial output; the status tells the caller
        const int64_t avail = (st < want ? st : want) - static_cast<int64_t>(r) * g.row_bytes;
        if (avail <= 0) continue;
        const int npx = avail >= g.row_bytes ? g.width : static_cast<int>(avail / (spp * f.bps));
        in += static_cast<int64_t>(r) * g.row_bytes;
        uint8_t* out = f.dst + row * out_row_bytes;
        if (f.bps == 8) {
            if (hm::aligned_dev(in, 8) && hm::aligned_dev(out, 8)) {
                const uint64_t* in8 = reinterpret_cast<const uint64_t*>(in);
                uint64_t* out8 = reinterpret_cast<uint64_t*>(out);
                for (int64_t e = lane; e < static_cast<int64_t>(npx) * ospp; e += hm::kWave) {
                    const int64_t px = e / ospp;
                    const int c = static_cast<int>(e - px * ospp);
                    out8[e] = in8[px * spp + src_channel(c, spp)];
                }
            } else {                                   // a strip at an odd file offset: byte by byte
                for (int64_t b = lane; b < static_cast<int64_t>(npx) * ospp * 8; b += hm::kWave) {
                    const int64_t e = b >> 3, px = e / ospp;
                    const int c = static_cast<int>(e - px * ospp);
                    out[b] = in[((px * spp + src_channel(c, spp)) << 3) + (b & 7)];
                }
            }
            continue;
        }
        uint32_t carry[4] = {0, 0, 0, 0};
        for (int x0 = 0; x0 < npx; x0 += hm::kWave) {
            const int px = x0 + lane;
            const bool act = px < npx;
            uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < spp && act) v[c] = in[static_cast<int64_t>(px) * spp + c];
            if (f.predictor == 2) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c < spp) {                     // wave-uniform
                        uint32_t x = v[c];
#pragma unroll
                        for (int d = 1; d < hm::kWave; d <<= 1) {
                            const uint32_t up = __shfl_up(x, d);
                            if (lane >= d) x += up;
                        }
                        x += carry[c];
                        carry[c] = __shfl(x, hm::kWave - 1) & 0xFFu;      // lanes past the row added 0: lane 63 holds the running sum
                        v[c] = x;
                    }
                }
            }
            if (act) {
                uint8_t* q = out + static_cast<int64_t>(px) * ospp;
                if (spp == 1) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (c < ospp) q[c] = static_cast<uint8_t>(v[0]);
                } else {
                    q[0] = static_cast<uint8_t>(v[2]);
                    q[1] = static_cast<uint8_t>(v[1]);
                    q[2] = static_cast<uint8_t>(v[0]);
                    if (ospp == 4) q[3] = static_cast<uint8_t>(v[3]);
                }
            }
        }
    }
}

struct WideGeom {
    StripGeom g;
    int compression, predictor, spp, big_endian, color_mode;
    uint8_t* dst;
};

// the wave as the lanes of hm_tiff_wide_body.h: 64 pixels per step
struct WaveLanes {
    int ln;
    __device__ __forceinline__ int width() const { return hm::kWave; }
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ uint32_t scan_add(uint32_t x) const {
#pragma unroll
        for (int d = 1; d < hm::kWave; d <<= 1) {
            const uint32_t up = __shfl_up(x, d);
            if (ln >= d) x += up;
        }
        return x;
    }
    __device__ __forceinline__ uint32_t last(uint32_t x) const { return __shfl(x, hm::kWave - 1); }
};

template <int B>
__global__ __launch_bounds__(256) void wide_rows_kernel(const WideGeom f) {
    const StripGeom& g = f.g;
    WaveLanes lanes{static_cast<int>(threadIdx.x & 63)};
    const int out_px_bytes = f.color_mode == 1 ? 3 : f.spp * B;
    const int64_t out_row_bytes = static_cast<int64_t>(g.width) * out_px_bytes;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); row < g.height; row += static_cast<int64_t>(gridDim.x) * 4) {
        const int s = static_cast<int>(row / g.rps);
        const int r = static_cast<int>(row - static_cast<int64_t>(s) * g.rps);
        const int rows_left = g.height - s * g.rps;
        const int64_t want = static_cast<int64_t>(rows_left < g.rps ? rows_left : g.rps) * g.row_bytes;
        const uint8_t* in;
        int64_t st;
        if (f.compression == 1) {
            const int64_t o = g.offsets[s], c = g.counts[s];
            st = strip_range_ok(o, c, g.file_len) ? (c < want ? c : want) : static_cast<int64_t>(HM_EINVAL);
            if (r == 0 && lanes.ln == 0) g.status[s] = st;
            in = g.file + o;
        } else {
            st = g.status[s];
            in = g.workspace + static_cast<int64_t>(s) * g.strip_bytes;
        }
        // failed and short strips: as in finish_rows_kernel. A stream that ends inside a sample or a pixel does not give that pixel
        const int64_t avail = (st < want ? st : want) - static_cast<int64_t>(r) * g.row_bytes;
        if (avail <= 0) continue;
        const int npx = avail >= g.row_bytes ? g.width : static_cast<int>(avail / (f.spp * B));
        hm_tiff_wide::finish_row<B>(in + static_cast<int64_t>(r) * g.row_bytes, npx, f.spp, f.big_endian != 0, f.predictor, f.color_mode,
                                    f.dst + row * out_row_bytes, lanes);
    }
}

}  // namespace

extern "C" size_t hm_tiff_decode_workspace_bytes(int n_strips, int64_t strip_bytes, int compression) {
    return hm_rules::tiff_decode_workspace_bytes(n_strips, strip_bytes, compression);
}

extern "C" int hm_tiff_decode_strips(const uint8_t* file, int64_t file_len, const int64_t* strip_offsets, const int64_t* strip_counts,
                                     int n_strips, int compression, int predictor, int rows_per_strip, int height, int width,
                                     int samples, int bytes_per_sample, int color_mode, void* dst, int64_t* strip_status,
                                     void* workspace, void* stream) {
    hm_rules::TiffDecodeGeom geom;
    const int rc = hm_rules::check_tiff_decode(file, file_len, strip_offsets, strip_counts, n_strips, compression, predictor, rows_per_strip,
                                               height, width, samples, bytes_per_sample, color_mode, dst, strip_status, workspace, geom);
    if (rc != HM_OK) return rc;
    const int64_t strip_bytes = geom.strip_bytes;
    hipStream_t st = hm::as_stream(stream);
    FinishGeom f;
    f.g = StripGeom{file, file_len, strip_offsets, strip_counts, n_strips, geom.rps, height, width, geom.row_bytes, strip_bytes, strip_status,
                    static_cast<uint8_t*>(workspace)};
    f.compression = compression;
    f.predictor = predictor;
    f.spp = samples;
    f.bps = bytes_per_sample;
    f.out_spp = color_mode == 1 ? 3 : samples;
    f.dst = static_cast<uint8_t*>(dst);
    if (compression == 5) {
        const unsigned grid = static_cast<unsigned>((n_strips + kLzwWaves - 1) / kLzwWaves);
        if (strip_bytes <= kStageBytes) hipLaunchKernelGGL(lzw_strips_kernel<true>, dim3(grid), dim3(kLzwWaves * hm::kWave), 0, st, f.g);
        else hipLaunchKernelGGL(lzw_strips_kernel<false>, dim3(grid), dim3(kLzwWaves * hm::kWave), 0, st, f.g);
        const int e = hm::launch_status();
        if (e != HM_OK) return e;
    }
    hipLaunchKernelGGL(finish_rows_kernel, dim3(hm::stream_grid(static_cast<int64_t>(height) * hm::kWave, 256, 8)), dim3(256), 0, st, f);
    return hm::launch_status();
}

extern "C" int hm_tiff_decode_strips_wide(const uint8_t* file, int64_t file_len, const int64_t* strip_offsets, const int64_t* strip_counts,
                                          int n_strips, int compression, int predictor, int rows_per_strip, int height, int width,
                                          int samples, int bytes_per_sample, int big_endian, int color_mode, void* dst,
                                          int64_t* strip_status, void* workspace, void* stream) {
    hm_rules::TiffDecodeGeom geom;
    const int rc = hm_rules::check_tiff_decode_wide(file, file_len, strip_offsets, strip_counts, n_strips, compression, predictor,
                                                    rows_per_strip, height, width, samples, bytes_per_sample, big_endian, color_mode, dst,
                                                    strip_status, workspace, geom);
    if (rc != HM_OK) return rc;
    hipStream_t st = hm::as_stream(stream);
    WideGeom f;
    f.g = StripGeom{file, file_len, strip_offsets, strip_counts, n_strips, geom.rps, height, width, geom.row_bytes, geom.strip_bytes,
                    strip_status, static_cast<uint8_t*>(workspace)};
    f.compression = compression;
    f.predictor = predictor;
    f.spp = samples;
    f.big_endian = big_endian;
    f.color_mode = color_mode;
    f.dst = static_cast<uint8_t*>(dst);
    if (compression == 5) {
        const unsigned grid = static_cast<unsigned>((n_strips + kLzwWaves - 1) / kLzwWaves);
        if (geom.strip_bytes <= kStageBytes) hipLaunchKernelGGL(lzw_strips_kernel<true>, dim3(grid), dim3(kLzwWaves * hm::kWave), 0, st, f.g);
        else hipLaunchKernelGGL(lzw_strips_kernel<false>, dim3(grid), dim3(kLzwWaves * hm::kWave), 0, st, f.g);
        const int e = hm::launch_status();
        if (e != HM_OK) return e;
    }
    const dim3 grid(hm::stream_grid(static_cast<int64_t>(height) * hm::kWave, 256, 8));
    if (bytes_per_sample == 2) hipLaunchKernelGGL(wide_rows_kernel<2>, grid, dim3(256), 0, st, f);
    else if (bytes_per_sample == 4) hipLaunchKernelGGL(wide_rows_kernel<4>, grid, dim3(256), 0, st, f);
    else hipLaunchKernelGGL(wide_rows_kernel<8>, grid, dim3(256), 0, st, f);
    return hm::launch_status();
}
