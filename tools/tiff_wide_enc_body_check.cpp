// tiff_wide_enc_body_check.cpp - host check of the wide TIFF pack row (camera_linearity_amd/csrc/hm_tiff_wide_enc_body.h, the row of
// hm_tiff_encode_strips_wide in both builds) under AddressSanitizer / UBSan. A development step for whoever changes that header: a
// stand-alone program, not part of the library or the package, and it needs no GPU (tests/test_tiff_encode_wide_host.py builds and runs it).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icamera_linearity_amd/csrc \
//       tools/tiff_wide_enc_body_check.cpp -o /tmp/tiff_wide_enc_body_check && /tmp/tiff_wide_enc_body_check
//
// Rows: the four source kinds (uint16, float32, float64 -> float32, float64 -> uint16) x 1 / 3 / 4 samples per pixel x Predictor 1 / 2
// (uint16 output) x 0, 1, 63, 64, 65, 129 and 3000 pixels - the test shapes' widths and one long row. The source is a heap block of
// exactly the row's source samples and the output a heap block of exactly the row's stored bytes, so any access outside them stops the
// program; UBSan stops it on a misaligned sample-wide access and on a float-to-integer cast out of range.
// Two forms of the lanes:
//   serial   one sample per step, what the host build runs;
//   wave     64 samples per step, run lane after lane: the addresses and the values are those of the device's wave (no lane depends
//            on another).
// Both are compared, byte for byte, with a reference written out here: the channel map spelled out per pixel, the stored value
// computed with the C library alone (nearbyint, a float cast), the difference to the left pixel taken on the stored values.
// Then the two formulas on their own: quantize_u16 on ties, negative, non-finite and huge samples, narrow_f32 on float32 subnormals,
// ties at the rounding boundary, overflow and NaN.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "hm_tiff_wide_enc_body.h"

namespace {

using namespace hm_tiff_wide_enc;

struct SerialLanes {
    int width() const { return 1; }
    int lane() const { return 0; }
};

struct OneLaneOfAWave {
    int ln;
    int width() const { return 64; }
    int lane() const { return ln; }
};

int src_bytes(int kind) { return kind == kSrcU16 ? 2 : (kind == kSrcF32 ? 4 : 8); }
int out_bytes_of(int kind) { return (kind == kSrcU16 || kind == kSrcF64AsU16) ? 2 : 4; }

template <class Lanes>
void run(int kind, const void* src, double divisor, int max_dn, int npx, int spp, int pred, uint8_t* out, Lanes& l) {
    if (out_bytes_of(kind) == 2) pack_row<2>(src, kind, divisor, max_dn, npx, spp, pred, out, l);
    else pack_row<4>(src, kind, divisor, max_dn, npx, spp, pred, out, l);
}

// the stored value of one source sample, with the C library alone
uint32_t stored_ref(int kind, const uint8_t* src, size_t at, double divisor, int max_dn) {
    if (kind == kSrcU16) { uint16_t v; memcpy(&v, src + at * 2, 2); return v; }
    if (kind == kSrcF32) { uint32_t v; memcpy(&v, src + at * 4, 4); return v; }
    double d;
    memcpy(&d, src + at * 8, 8);
    if (kind == kSrcF64AsF32) { const float f = static_cast<float>(d); uint32_t v; memcpy(&v, &f, 4); return v; }
    const double r = nearbyint((d / divisor) * max_dn);
    if (!std::isfinite(r) || std::fabs(r) >= 9223372036854775808.0) return 0;
    return static_cast<uint32_t>(static_cast<uint64_t>(static_cast<long long>(r)) & 0xFFFFu);
}

std::vector<uint8_t> reference(int kind, const uint8_t* src, double divisor, int max_dn, int npx, int spp, int pred) {
    const int B = out_bytes_of(kind);
    std::vector<uint8_t> out(static_cast<size_t>(npx) * spp * B);
    for (int px = 0; px < npx; ++px)
        for (int c = 0; c < spp; ++c) {
            const int sc = spp == 1 ? 0 : (c == 0 ? 2 : (c == 2 ? 0 : c));       // file R <- memory channel 2, B <- 0, G and A stay
            uint32_t v = stored_ref(kind, src, static_cast<size_t>(px) * spp + sc, divisor, max_dn);
            if (pred == 2 && px > 0) v = (v - stored_ref(kind, src, static_cast<size_t>(px - 1) * spp + sc, divisor, max_dn)) & 0xFFFFu;
            memcpy(&out[(static_cast<size_t>(px) * spp + c) * B], &v, B);       // little-endian host, like the library
        }
    return out;
}

long n_rows = 0;

void check(std::mt19937_64& rng, int kind, int spp, int pred, int npx, double divisor, int max_dn) {
    const size_t n = static_cast<size_t>(npx) * spp;
    const size_t in_bytes = n * src_bytes(kind), out_bytes = n * out_bytes_of(kind);
    uint8_t* src = static_cast<uint8_t*>(malloc(in_bytes ? in_bytes : 1));        // exactly the row: ASan's red zone follows
    if (kind == kSrcU16 || kind == kSrcF32) {
        for (size_t k = 0; k < in_bytes; ++k) src[k] = static_cast<uint8_t>(rng());
        static const uint16_t edge[5] = {0, 65535, 1, 32768, 32767};             // differences that wrap both ways
        if (kind == kSrcU16) for (size_t k = 0; k < n && k < 40; ++k) memcpy(src + 2 * k, &edge[(k / spp) % 5], 2);
    } else {
        std::uniform_real_distribution<double> u(-0.25, 1.25);
        for (size_t k = 0; k < n; ++k) {
            double d = u(rng) * divisor;
            if (k % 97 == 5) d = std::numeric_limits<double>::quiet_NaN();
            if (k % 97 == 6) d = std::numeric_limits<double>::infinity();
            if (k % 97 == 7) d = -1e300;
            if (k % 97 == 8) d = 3e-42;                                            // a float32 subnormal
            if (k % 97 == 9) d = (k % 1000 + 0.5) / max_dn * divisor;              // near a tie
            memcpy(src + 8 * k, &d, 8);
        }
    }
    uint8_t* a = static_cast<uint8_t*>(malloc(out_bytes ? out_bytes : 1));
    uint8_t* w = static_cast<uint8_t*>(malloc(out_bytes ? out_bytes : 1));
    memset(a, 0xEE, out_bytes);
    memset(w, 0xEE, out_bytes);
    SerialLanes serial;
    run(kind, src, divisor, max_dn, npx, spp, pred, a, serial);
    for (int l = 0; l < 64; ++l) {
        OneLaneOfAWave lane{l};
        run(kind, src, divisor, max_dn, npx, spp, pred, w, lane);
    }
    const std::vector<uint8_t> want = reference(kind, src, divisor, max_dn, npx, spp, pred);
    bool ok = want.size() == out_bytes;
    if (ok && kind == kSrcF64AsF32) {           // a NaN stays a NaN; its payload bits are not pinned
        for (size_t k = 0; k < n && ok; ++k) {
            uint32_t x, y, z;
            memcpy(&x, &want[4 * k], 4); memcpy(&y, a + 4 * k, 4); memcpy(&z, w + 4 * k, 4);
            const bool nan = (x & 0x7FFFFFFFu) > 0x7F800000u;
            ok = nan ? ((y & 0x7FFFFFFFu) > 0x7F800000u && (z & 0x7FFFFFFFu) > 0x7F800000u) : (x == y && x == z);
        }
    } else if (ok && out_bytes) {
        ok = memcmp(a, want.data(), out_bytes) == 0 && memcmp(w, want.data(), out_bytes) == 0;
    }
    if (!ok) {
        fprintf(stderr, "MISMATCH: kind %d spp %d pred %d npx %d divisor %g max_dn %d\n", kind, spp, pred, npx, divisor, max_dn);
        exit(1);
    }
    ++n_rows;
    free(src); free(a); free(w);
}

void expect(const char* what, uint32_t got, uint32_t want) {
    if (got != want) { fprintf(stderr, "%s: got %u, want %u\n", what, got, want); exit(1); }
}

uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

}  // namespace

int main() {
    std::mt19937_64 rng(11);
    for (int kind = 0; kind < 4; ++kind)
        for (int spp : {1, 3, 4})
            for (int pred = 1; pred <= (out_bytes_of(kind) == 2 ? 2 : 1); ++pred)
                for (int npx : {0, 1, 63, 64, 65, 129, 3000})
                    for (int max_dn : {511, 4095, 65535})
                        for (double divisor : {1.0, 3.7}) {
                            if (kind != kSrcF64AsU16 && (max_dn != 511 || divisor != 1.0)) continue;
                            check(rng, kind, spp, pred, npx, divisor, max_dn);
                        }
    // quantize_u16: halves to even, negative results wrap, what cannot be an int64 gives 0
    expect("q 0.5/4095", quantize_u16(0.5 / 4095.0, 1.0, 4095), static_cast<uint32_t>(nearbyint((0.5 / 4095.0) * 4095.0)));
    expect("q 2.5 -> 2", quantize_u16(2.5, 1.0, 1), 2);
    expect("q 3.5 -> 4", quantize_u16(3.5, 1.0, 1), 4);
    expect("q -1", quantize_u16(-1.0 / 4095.0, 1.0, 4095), 65535);
    expect("q max_dn + 1", quantize_u16(4096.0 / 4095.0, 1.0, 4095), 4096);
    expect("q 65536 wraps", quantize_u16(65536.0 / 65535.0, 1.0, 65535), 0);
    expect("q nan", quantize_u16(std::numeric_limits<double>::quiet_NaN(), 1.0, 4095), 0);
    expect("q inf", quantize_u16(std::numeric_limits<double>::infinity(), 1.0, 4095), 0);
    expect("q -inf", quantize_u16(-std::numeric_limits<double>::infinity(), 1.0, 4095), 0);
    expect("q 1e300", quantize_u16(1e300, 1.0, 4095), 0);
    expect("q 2^63", quantize_u16(9223372036854775808.0, 1.0, 1), 0);
    expect("q 2^62", quantize_u16(4611686018427387904.0, 1.0, 1), 0);               // a multiple of 65536
    expect("q 2^62 + 2^10", quantize_u16(4611686018427387904.0 + 1024.0, 1.0, 1), 1024);
    // narrow_f32: subnormals kept, ties to even, overflow, zeros, NaN
    const double tiny = std::ldexp(1.0, -149);                                       // the smallest float32 subnormal
    expect("n tiny", narrow_f32(tiny), 1);
    expect("n tiny / 2 (tie -> 0)", narrow_f32(tiny * 0.5), 0);
    expect("n tiny * 1.5 (tie -> 2)", narrow_f32(tiny * 1.5), 2);
    expect("n tiny * 2.5 (tie -> 2)", narrow_f32(tiny * 2.5), 2);
    expect("n -tiny", narrow_f32(-tiny), 0x80000001u);
    expect("n 1 + 2^-24 (tie -> 1)", narrow_f32(1.0 + std::ldexp(1.0, -24)), bits_of(1.0f));
    expect("n 1 + 3 * 2^-24 (tie -> 1 + 2^-22)", narrow_f32(1.0 + 3 * std::ldexp(1.0, -24)), bits_of(1.0f) + 2);
    expect("n 1e39", narrow_f32(1e39), 0x7F800000u);
    expect("n -1e39", narrow_f32(-1e39), 0xFF800000u);
    expect("n max + half ulp (tie -> inf)", narrow_f32(std::ldexp(2.0 - std::ldexp(1.0, -24), 127)), 0x7F800000u);
    expect("n -0", narrow_f32(-0.0), 0x80000000u);
    expect("n nan", (narrow_f32(std::numeric_limits<double>::quiet_NaN()) & 0x7FFFFFFFu) > 0x7F800000u, 1);
    printf("tiff wide enc body check: %ld rows, serial and wave lanes, all equal to the reference; both formulas hold\n", n_rows);
    return 0;
}
