// tiff_wide_body_check.cpp - host check of the wide TIFF row pass (camera_linearity_amd/csrc/hm_tiff_wide_body.h, the row of
// hm_tiff_decode_strips_wide in both builds) under AddressSanitizer / UBSan. A development step for whoever changes that header: a
// stand-alone program, not part of the library, the package or the test suite, and it needs no GPU.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icamera_linearity_amd/csrc \
//       tools/tiff_wide_body_check.cpp -o /tmp/tiff_wide_body_check && /tmp/tiff_wide_body_check
//
// Rows: 2-, 4- and 8-byte samples x 1 / 3 / 4 samples per pixel x either byte order x Predictor 1 / 2 and both colour modes (2-byte
// samples) x 0, 1, 63, 64, 65, 129 and 3000 pixels x a row that starts 0, 1, 2, 3, 4 and 7 bytes off the 16-byte grid (aligned,
// odd, and aligned for some sample sizes only) x a tail of 0, 1, 3 and 7 bytes behind the last whole pixel (a short strip: the callers
// hand the body avail / pixel_bytes pixels, and the tail must not be read). The input is a heap block that ends with the row (and
// its tail), the output a heap block of exactly the pixels' bytes, so any access outside them stops the program; UBSan stops it on a
// misaligned sample-wide load.
// Two forms of the lanes:
//   serial   one pixel per step, what the host build runs: every output byte is compared with a reference written out here (bytes
//            assembled one by one, a running sum per sample modulo 65536, the channel map spelled out);
//   wave     64 pixels per step, run lane after lane with a scan that adds nothing: the addresses are those of the device's wave (they
//            do not depend on the values), the values are right where there is no predictor and compared there.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "hm_tiff_wide_body.h"

namespace {

struct SerialLanes {
    int width() const { return 1; }
    int lane() const { return 0; }
    uint32_t scan_add(uint32_t x) const { return x; }
    uint32_t last(uint32_t x) const { return x; }
};

struct OneLaneOfAWave {                  // addresses only: see above
    int ln;
    int width() const { return 64; }
    int lane() const { return ln; }
    uint32_t scan_add(uint32_t x) const { return x; }
    uint32_t last(uint32_t x) const { return x; }
};

template <int B, class Lanes>
void run(const uint8_t* in, int npx, int spp, bool be, int pred, int color, uint8_t* out, Lanes& l) {
    hm_tiff_wide::finish_row<B>(in, npx, spp, be, pred, color, out, l);
}

template <class Lanes>
void run_b(int B, const uint8_t* in, int npx, int spp, bool be, int pred, int color, uint8_t* out, Lanes& l) {
    if (B == 2) run<2>(in, npx, spp, be, pred, color, out, l);
    else if (B == 4) run<4>(in, npx, spp, be, pred, color, out, l);
    else run<8>(in, npx, spp, be, pred, color, out, l);
}

// the reference: the row cv.imread gives, byte by byte
std::vector<uint8_t> reference(const uint8_t* in, int npx, int spp, int B, bool be, int pred, int color) {
    const int ospp = color ? 3 : spp;
    std::vector<uint8_t> out(static_cast<size_t>(npx) * (color ? 3 : spp * B));
    uint64_t sum[4] = {0, 0, 0, 0};
    for (int px = 0; px < npx; ++px) {
        uint64_t v[4] = {0, 0, 0, 0};
        for (int c = 0; c < spp; ++c) {
            const uint8_t* p = in + (static_cast<size_t>(px) * spp + c) * B;
            for (int k = 0; k < B; ++k) v[c] |= static_cast<uint64_t>(p[k]) << (8 * (be ? B - 1 - k : k));
            if (pred == 2) v[c] = sum[c] = (sum[c] + v[c]) & 0xFFFF;
        }
        for (int c = 0; c < ospp; ++c) {
            const uint64_t x = v[spp == 1 ? 0 : (c < 3 ? 2 - c : c)];
            if (color) out[static_cast<size_t>(px) * 3 + c] = static_cast<uint8_t>(x >> 8);
            else memcpy(&out[(static_cast<size_t>(px) * ospp + c) * B], &x, B);       // little-endian host, like the library
        }
    }
    return out;
}

long n_rows = 0;

void check(std::mt19937& rng, int B, int spp, bool be, int pred, int color, int npx, int off, int tail) {
    const size_t in_bytes = static_cast<size_t>(npx) * spp * B + tail;
    const size_t out_bytes = static_cast<size_t>(npx) * (color ? 3 : spp * B);
    uint8_t* block = static_cast<uint8_t*>(malloc(off + in_bytes + (off + in_bytes == 0)));    // ends with the row: ASan's red zone follows
    uint8_t* in = block + off;
    for (size_t k = 0; k < in_bytes; ++k) in[k] = static_cast<uint8_t>(rng());
    uint8_t* a = static_cast<uint8_t*>(malloc(out_bytes ? out_bytes : 1));
    uint8_t* w = static_cast<uint8_t*>(malloc(out_bytes ? out_bytes : 1));
    memset(a, 0xEE, out_bytes);
    memset(w, 0xEE, out_bytes);
    const int avail_px = static_cast<int>(in_bytes / (static_cast<size_t>(spp) * B));        // what the callers compute for a short strip
    if (avail_px != npx) { fprintf(stderr, "the tail holds a whole pixel\n"); exit(1); }
    SerialLanes serial;
    run_b(B, in, npx, spp, be, pred, color, a, serial);
    for (int l = 0; l < 64; ++l) {
        OneLaneOfAWave lane{l};
        run_b(B, in, npx, spp, be, pred, color, w, lane);
    }
    const std::vector<uint8_t> want = reference(in, npx, spp, B, be, pred, color);
    auto same = [&](const uint8_t* got) { return out_bytes == 0 || memcmp(got, want.data(), out_bytes) == 0; };
    if (want.size() != out_bytes || !same(a) || (pred == 1 && !same(w))) {
        fprintf(stderr, "MISMATCH: B %d spp %d be %d pred %d color %d npx %d off %d tail %d\n", B, spp, be, pred, color, npx, off, tail);
        exit(1);
    }
    ++n_rows;
    free(block); free(a); free(w);
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    for (int B : {2, 4, 8})
        for (int spp : {1, 3, 4})
            for (int be = 0; be < 2; ++be)
                for (int pred = 1; pred <= (B == 2 ? 2 : 1); ++pred)
                    for (int color = 0; color <= (B == 2 ? 1 : 0); ++color)
                        for (int npx : {0, 1, 63, 64, 65, 129, 3000})
                            for (int off : {0, 1, 2, 3, 4, 7})
                                for (int tail : {0, 1, 3, 7})
                                    if (tail < spp * B) check(rng, B, spp, be != 0, pred, color, npx, off, tail);
    printf("tiff wide body check: %ld rows, serial and wave lanes, all equal to the reference\n", n_rows);
    return 0;
}
