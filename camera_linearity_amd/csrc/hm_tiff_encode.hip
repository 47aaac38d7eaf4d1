// hm_tiff_encode.hip - TIFF strips encoded on the device: hm_tiff_encode_strips (include/hdrmerge.h), the writing twin of
// hm_tiff_device.hip. One call turns an image in device memory into the strips of a TIFF file, ready to be copied down once.
//
//   pack_rows_kernel    The inverse of finish_rows_kernel. One row per wave, 64 pixels per step: reads (H, W, S) in B,G,R(,A) order,
//                       optionally quantises float64 to uint8 (hm_lzw_enc::quantize_u8: save_8bit's arithmetic), swaps R and B, applies
//                       Predictor 2 (a difference to the pixel on the left, which is read again from the source: no scan) and writes
//                       file order. Compression 1 writes straight into the payload at s * strip_bytes and is the only kernel of that
//                       path; compression 5 writes the strip's slot of the workspace.
//   wide_pack_rows_kernel  pack_rows_kernel for hm_tiff_encode_strips_wide: 2- and 4-byte stored samples (uint16 as it is, float32 bit for
//                       bit, float64 narrowed to float32 or quantised to uint16), the same geometry - one row per wave, 64 pixels per
//                       spp steps, a grid-stride loop over rows - and the same two destinations. The row is hm_tiff_wide_enc_body.h,
//                       the text the host build runs too: the lanes of a step store 64 CONSECUTIVE samples (one run of 128 or 256
//                       bytes per wave store, whatever the pixel size) and gather their source samples from the same run.
//   lzw_encode_kernel   One strip per WAVE, one wave per workgroup. The encoder state (prefix, next, code width, bit accumulator) is
//                       wave-uniform and every lane runs the same loop of hm_tiff_lzw_enc_body.h. The lanes do what is parallel: the
//                       input is fetched 256 bytes at a time (one dword per lane, the next chunk in flight while this one is consumed,
//                       so no strip has to fit a staging buffer), the dictionary is probed 64 consecutive slots at once (one LDS round
//                       trip, a ballot for the match and one for the first free slot), a Clear empties it with 16-byte LDS stores, and
//                       finished output words wait in one register per lane and leave 256 bytes at a time, coalesced.
//                       LDS per wave: the dictionary, 8192 x 4 B = 32 KiB, nothing else. 160 KiB per CU hold 5 such workgroups: 5 waves
//                       of the 32 a CU can hold. LDS bounds occupancy, and the loop is latency-bound (one dependent LDS round trip per
//                       input byte), not bandwidth-bound. Measured figures: DESIGN.md 4.4.6.
//   scan_counts_kernel  One workgroup: exclusive scan of the strip byte counts, each rounded up to 16, looping with a carry.
//   compact_kernel      One workgroup per strip (both per-strip kernels loop where an image has more than 2^16 strips): 16-byte moves from the strip's slot to payload + strip_offsets[s]; the bytes between
//                       the end of a stream and the next multiple of 16 are written as zeros, so every byte of payload[0, total) is
//                       defined by the call.
//
// Safety: every store of pack_rows_kernel lies in its row of its strip; the encoder's bounds are those stated in
// hm_tiff_lzw_enc_body.h with cap = hm_lzw_enc::bound(strip bytes) <= the slot's pitch; compact_kernel reads [0, round_up(count, 16)) of
// a slot whose pitch is round_up(bound, 16) and writes [offset, offset + round_up(count, 16)), and the offsets sum to at most
// n_strips * pitch = hm_tiff_encode_payload_bytes <= payload_cap. No atomics, no allocation, no host synchronisation.
#include "hm_common.h"
#include "hm_tiff_lzw_enc_body.h"
#include "hm_tiff_rules.h"
#include "hm_tiff_wide_enc_body.h"

static_assert(int(hm_lzw_enc::kEshape) == int(HM_ESHAPE), "hm_tiff_lzw_enc_body.h repeats a code of hdrmerge.h");

namespace {

constexpr int kMaxStripGrid = 1 << 16;       // workgroups of the per-strip kernels: an image of more strips (up to 2^31 - 1 one-row strips) loops

using hm_rules::round16;

struct EncGeom {
    const uint8_t* src;
    int kind;                                // 0 uint8, 1 float64, 2 float64 -> uint8; the wide entry: HM_TIFF_SRC_* (0 .. 3)
    double divisor;
    int height, width, spp;
    int rps;                                 // rows per strip, already clamped to the height
    int n_strips;
    int compression, predictor;
    int out_bps;                             // bytes per stored sample: 1 or 8; the wide entry: 2 or 4
    int64_t row_bytes;                       // of the stored layout
    int64_t strip_bytes;                     // rps * row_bytes
    int64_t in_pitch;                        // compression 5: round16(strip_bytes), the pitch of the packed strips in the workspace
    int64_t out_pitch;                       // compression 5: round16(bound(strip_bytes)), the pitch of the streams behind them
    int64_t bound;                           // hm_lzw_enc::bound(strip_bytes)
    uint8_t* payload;
    int64_t* offsets;                        // n_strips + 1
    int64_t* counts;                         // n_strips
    uint8_t* workspace;
};

__device__ __forceinline__ int file_channel(int c, int spp) { return spp >= 3 ? (c < 3 ? 2 - c : c) : 0; }

__device__ __forceinline__ int64_t strip_len(const EncGeom& g, int s) {
    const int rows_left = g.height - s * g.rps;
    return static_cast<int64_t>(rows_left < g.rps ? rows_left : g.rps) * g.row_bytes;
}

__global__ __launch_bounds__(256) void pack_rows_kernel(const EncGeom g) {
    const int lane = threadIdx.x & 63;
    const int spp = g.spp;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); row < g.height; row += static_cast<int64_t>(gridDim.x) * 4) {
        const int s = static_cast<int>(row / g.rps);
        const int r = static_cast<int>(row - static_cast<int64_t>(s) * g.rps);
        uint8_t* out = (g.compression == 1 ? g.payload + static_cast<int64_t>(s) * g.strip_bytes
                                           : g.workspace + static_cast<int64_t>(s) * g.in_pitch) + static_cast<int64_t>(r) * g.row_bytes;
        if (g.compression == 1 && r == 0 && lane == 0) {           // the tables of an uncompressed file: known from the geometry
            g.offsets[s] = static_cast<int64_t>(s) * g.strip_bytes;
            g.counts[s] = strip_len(g, s);
            if (s == g.n_strips - 1) g.offsets[g.n_strips] = static_cast<int64_t>(g.height) * g.row_bytes;
        }
        const int64_t in_row = row * g.width * spp;                // in samples
        if (g.kind == 1) {
            const uint64_t* in8 = reinterpret_cast<const uint64_t*>(g.src) + in_row;
            uint64_t* out8 = reinterpret_cast<uint64_t*>(out);
            for (int64_t e = lane; e < static_cast<int64_t>(g.width) * spp; e += hm::kWave) {
                const int64_t px = e / spp;
                const int c = static_cast<int>(e - px * spp);
                out8[e] = in8[px * spp + file_channel(c, spp)];
            }
            continue;
        }
        const uint8_t* in1 = g.src + in_row;
        const double* inf = reinterpret_cast<const double*>(g.src) + in_row;
        for (int x0 = 0; x0 < g.width; x0 += hm::kWave) {
            const int px = x0 + lane;
            if (px >= g.width) continue;
            uint8_t* q = out + static_cast<int64_t>(px) * spp;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c >= spp) break;
                const int64_t at = static_cast<int64_t>(px) * spp + file_channel(c, spp);
                uint32_t v, left = 0;
                if (g.kind == 0) {
                    v = in1[at];
                    if (g.predictor == 2 && px > 0) left = in1[at - spp];
                } else {
                    v = hm_lzw_enc::quantize_u8(inf[at], g.divisor);
                    if (g.predictor == 2 && px > 0) left = hm_lzw_enc::quantize_u8(inf[at - spp], g.divisor);
                }
                q[c] = static_cast<uint8_t>(v - left);
            }
        }
    }
}

struct WaveLanes {                           // the lanes of hm_tiff_wide_enc_body.h: one stored sample per lane and step
    int ln;
    __device__ __forceinline__ int width() const { return hm::kWave; }
    __device__ __forceinline__ int lane() const { return ln; }
};

// max_dn is an argument of its own: EncGeom, and with it the kernels above and below, stay as they were
__global__ __launch_bounds__(256) void wide_pack_rows_kernel(const EncGeom g, const int max_dn) {
    WaveLanes lanes{static_cast<int>(threadIdx.x & 63)};
    const int in_bps = g.kind == HM_TIFF_SRC_U16 ? 2 : (g.kind == HM_TIFF_SRC_F32 ? 4 : 8);
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); row < g.height; row += static_cast<int64_t>(gridDim.x) * 4) {
        const int s = static_cast<int>(row / g.rps);
        const int r = static_cast<int>(row - static_cast<int64_t>(s) * g.rps);
        uint8_t* out = (g.compression == 1 ? g.payload + static_cast<int64_t>(s) * g.strip_bytes
                                           : g.workspace + static_cast<int64_t>(s) * g.in_pitch) + static_cast<int64_t>(r) * g.row_bytes;
        if (g.compression == 1 && r == 0 && lanes.ln == 0) {       // the tables of an uncompressed file: known from the geometry
            g.offsets[s] = static_cast<int64_t>(s) * g.strip_bytes;
            g.counts[s] = strip_len(g, s);
            if (s == g.n_strips - 1) g.offsets[g.n_strips] = static_cast<int64_t>(g.height) * g.row_bytes;
        }
        const uint8_t* in = g.src + row * g.width * g.spp * in_bps;
        if (g.out_bps == 2) hm_tiff_wide_enc::pack_row<2>(in, g.kind, g.divisor, max_dn, g.width, g.spp, g.predictor, out, lanes);
        else hm_tiff_wide_enc::pack_row<4>(in, g.kind, g.divisor, max_dn, g.width, g.spp, g.predictor, out, lanes);
    }
}

// the wave's ops (hm_tiff_lzw_enc_body.h): all lanes call every function with the same arguments
struct WaveOps {
    int lane;
    int64_t n;                               // the strip's bytes
    int64_t chunk;                           // the 256-byte chunk `cur` holds, -1 before the first
    uint32_t cur, ahead;                     // this lane's dword of chunk `chunk` and of chunk + 1
    uint32_t mine;                           // the finished output word this lane holds until 64 of them leave together

    __device__ __forceinline__ uint32_t load(const uint8_t* src, int64_t c) const {
        const int64_t at = c * 256 + lane * 4;                     // src is 16-byte aligned and its slot holds round16(n) bytes
        return at < n ? *reinterpret_cast<const uint32_t*>(src + at) : 0u;
    }
    __device__ __forceinline__ uint8_t byte(const uint8_t* src, int64_t i) {
        const int64_t c = i >> 8;
        if (c != chunk) {                                          // wave-uniform: i rises by one per call
            cur = (chunk >= 0 && c == chunk + 1) ? ahead : load(src, c);
            ahead = load(src, c + 1);
            chunk = c;
        }
        const uint32_t w = __builtin_amdgcn_readlane(cur, __builtin_amdgcn_readfirstlane(static_cast<int>((i >> 2) & 63)));
        return static_cast<uint8_t>(w >> ((i & 3) * 8));
    }
    __device__ __forceinline__ void clear(hm_lzw_enc::Dict& d) {
        uint4* p = reinterpret_cast<uint4*>(d.slot);
        for (int k = lane; k < hm_lzw_enc::kSlots / 4; k += hm::kWave) p[k] = make_uint4(0, 0, 0, 0);
        __threadfence_block();
    }
    __device__ __forceinline__ int probe(const hm_lzw_enc::Dict& d, uint32_t start, uint32_t key, uint32_t* free_slot) const {
        const uint32_t e = d.slot[(start + lane) & (hm_lzw_enc::kSlots - 1)];
        const unsigned long long hit = __ballot(e != 0 && (e >> 12) == key);
        const unsigned long long empty = __ballot(e == 0);
        const int first_hit = hit ? __ffsll(hit) - 1 : 64, first_empty = empty ? __ffsll(empty) - 1 : 64;
        if (first_hit < first_empty)             // the ballots are wave-uniform, so the winner's word is a lane read, not a second LDS trip
            return static_cast<int>(__builtin_amdgcn_readlane(e, __builtin_amdgcn_readfirstlane(first_hit)) & 0xFFFu);
        if (first_empty < 64) { *free_slot = (start + first_empty) & (hm_lzw_enc::kSlots - 1); return -1; }
        return -2;
    }
    __device__ __forceinline__ void insert(hm_lzw_enc::Dict& d, uint32_t slot, uint32_t word) const {
        if (lane == 0) d.slot[slot] = word;
        __threadfence_block();               // the next probe's lanes read what lane 0 wrote
    }
    __device__ __forceinline__ void word(uint8_t* out, int64_t w, uint32_t v) {
        const int k = static_cast<int>(w & 63);
        if (lane == k) mine = v;
        if (k == 63) reinterpret_cast<uint32_t*>(out)[w - 63 + lane] = mine;
    }
    __device__ __forceinline__ void flush(uint8_t* out, int64_t n_words) const {
        const int k = static_cast<int>(n_words & 63);
        if (lane < k) reinterpret_cast<uint32_t*>(out)[n_words - k + lane] = mine;
    }
};

__global__ __launch_bounds__(hm::kWave) void lzw_encode_kernel(const EncGeom g) {
    __shared__ hm_lzw_enc::Dict dict;
    const int lane = threadIdx.x;
    for (int64_t s64 = blockIdx.x; s64 < g.n_strips; s64 += gridDim.x) {      // the grid is capped at kMaxStripGrid: images of more strips loop
        const int s = static_cast<int>(s64);
        const int64_t n = strip_len(g, s);
        const uint8_t* in = g.workspace + s64 * g.in_pitch;
        uint8_t* out = g.workspace + static_cast<int64_t>(g.n_strips) * g.in_pitch + s64 * g.out_pitch;
        WaveOps ops{lane, n, -1, 0u, 0u, 0u};
        const int64_t r = hm_lzw_enc::encode(in, n, out, g.bound, dict, ops);      // starts by emptying the dictionary
        if (lane == 0) g.counts[s] = r;      // the stream's bytes; HM_ESHAPE if it would have passed the bound (it cannot)
    }
}

__global__ __launch_bounds__(256) void scan_counts_kernel(const EncGeom g) {
    __shared__ int64_t part[256];
    __shared__ int64_t carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < g.n_strips; base += 256) {
        const int s = base + t;
        const int64_t c = s < g.n_strips ? g.counts[s] : 0;
        const int64_t mine = c > 0 ? round16(c) : 0;
        part[t] = mine;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t add = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        const int64_t before = carry + part[t] - mine;             // exclusive
        if (s < g.n_strips) g.offsets[s] = before;
        __syncthreads();
        if (t == 255) carry += part[255];
        __syncthreads();
    }
    if (t == 0) g.offsets[g.n_strips] = carry;
}

__global__ __launch_bounds__(256) void compact_kernel(const EncGeom g) {
    for (int64_t s = blockIdx.x; s < g.n_strips; s += gridDim.x) {
        const int64_t c = g.counts[s];
        if (c <= 0) continue;
        const uint4* in = reinterpret_cast<const uint4*>(g.workspace + static_cast<int64_t>(g.n_strips) * g.in_pitch + s * g.out_pitch);
        uint4* out = reinterpret_cast<uint4*>(g.payload + g.offsets[s]);
        const int64_t units = round16(c) >> 4;
        for (int64_t u = threadIdx.x; u < units; u += blockDim.x) {
            uint4 v = in[u];
            const int64_t keep = c - (u << 4);                     // bytes of this unit that belong to the stream
            if (keep < 16) {
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t kb = keep - 4 * k;               // bytes of word k to keep
                    if (kb <= 0) w[k] = 0;
                    else if (kb < 4) w[k] &= (1u << (8 * kb)) - 1u;
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            out[u] = v;
        }
    }
}

}  // namespace

extern "C" int64_t hm_tiff_encode_bound(int64_t strip_bytes) { return hm_rules::tiff_encode_bound(strip_bytes); }

extern "C" size_t hm_tiff_encode_workspace_bytes(int n_strips, int64_t strip_bytes, int compression) {
    return hm_rules::tiff_encode_workspace_bytes(n_strips, strip_bytes, compression);
}

extern "C" size_t hm_tiff_encode_payload_bytes(int n_strips, int64_t strip_bytes, int compression) {
    return hm_rules::tiff_encode_payload_bytes(n_strips, strip_bytes, compression);
}

namespace {

EncGeom make_geom(const hm_rules::TiffEncodeGeom& v, const void* src, int src_kind, double divisor, int height, int width, int samples,
                  int compression, int predictor, void* payload, void* strip_offsets, void* strip_counts, void* workspace) {
    EncGeom g{};
    g.kind = src_kind; g.divisor = divisor; g.height = height; g.width = width; g.spp = samples;
    g.rps = v.rps; g.n_strips = v.n_strips; g.compression = compression; g.predictor = predictor; g.out_bps = v.out_bps;
    g.row_bytes = v.row_bytes; g.strip_bytes = v.strip_bytes; g.in_pitch = v.in_pitch; g.out_pitch = v.out_pitch; g.bound = v.bound;
    g.src = static_cast<const uint8_t*>(src);
    g.payload = static_cast<uint8_t*>(payload);
    g.offsets = static_cast<int64_t*>(strip_offsets);
    g.counts = static_cast<int64_t*>(strip_counts);
    g.workspace = static_cast<uint8_t*>(workspace);
    return g;
}

// what follows the pack kernel with Compression 5, the same for both entries: the strips' slots of the workspace -> payload and tables
int launch_lzw_stage(const EncGeom& g, hipStream_t st) {
    int e;
    const unsigned strip_grid = static_cast<unsigned>(g.n_strips < kMaxStripGrid ? g.n_strips : kMaxStripGrid);
    hipLaunchKernelGGL(lzw_encode_kernel, dim3(strip_grid), dim3(hm::kWave), 0, st, g);
    if ((e = hm::launch_status()) != HM_OK) return e;
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(256), 0, st, g);
    if ((e = hm::launch_status()) != HM_OK) return e;
    hipLaunchKernelGGL(compact_kernel, dim3(strip_grid), dim3(256), 0, st, g);
    return hm::launch_status();
}

}  // namespace

extern "C" int hm_tiff_encode_strips(const void* src, int src_kind, double divisor, int height, int width, int samples, int rows_per_strip,
                                     int compression, int predictor, void* payload, int64_t payload_cap, void* strip_offsets,
                                     void* strip_counts, void* workspace, void* stream) {
    hm_rules::TiffEncodeGeom v;
    const int rc = hm_rules::check_tiff_encode(src, src_kind, divisor, height, width, samples, rows_per_strip, compression, predictor, payload,
                                               payload_cap, strip_offsets, strip_counts, workspace, v);
    if (rc != HM_OK) return rc;
    const EncGeom g = make_geom(v, src, src_kind, divisor, height, width, samples, compression, predictor, payload, strip_offsets, strip_counts,
                                workspace);
    hipStream_t st = hm::as_stream(stream);
    hipLaunchKernelGGL(pack_rows_kernel, dim3(hm::stream_grid(static_cast<int64_t>(height) * hm::kWave, 256, 8)), dim3(256), 0, st, g);
    const int e = hm::launch_status();
    if (e != HM_OK || compression == 1) return e;
    return launch_lzw_stage(g, st);
}

// The pack launch: at most cu_count() * 8 workgroups of 4 waves, one row per wave - taller images run the grid-stride row loop.
extern "C" int hm_tiff_encode_strips_wide(const void* src, int src_kind, double divisor, int max_dn, int height, int width, int samples,
                                          int rows_per_strip, int compression, int predictor, void* payload, int64_t payload_cap,
                                          void* strip_offsets, void* strip_counts, void* workspace, void* stream) {
    hm_rules::TiffEncodeGeom v;
    const int rc = hm_rules::check_tiff_encode_wide(src, src_kind, divisor, max_dn, height, width, samples, rows_per_strip, compression, predictor,
                                                    payload, payload_cap, strip_offsets, strip_counts, workspace, v);
    if (rc != HM_OK) return rc;
    const EncGeom g = make_geom(v, src, src_kind, divisor, height, width, samples, compression, predictor, payload, strip_offsets, strip_counts,
                                workspace);
    hipStream_t st = hm::as_stream(stream);
    hipLaunchKernelGGL(wide_pack_rows_kernel, dim3(hm::stream_grid(static_cast<int64_t>(height) * hm::kWave, 256, 8)), dim3(256), 0, st, g, max_dn);
    const int e = hm::launch_status();
    if (e != HM_OK || compression == 1) return e;
    return launch_lzw_stage(g, st);
}
