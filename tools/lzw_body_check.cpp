// lzw_body_check.cpp - host check of the device LZW decoder's body (camera_linearity_amd/csrc/hm_tiff_lzw_body.h) under
// AddressSanitizer / UBSan. A development step for whoever changes that header: a stand-alone program, not part of the library, the
// package or the test suite, and it needs no GPU.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icamera_linearity_amd/csrc \
//       -x c++ tools/lzw_body_check.cpp camera_linearity_amd/csrc/hm_tiff.hip -o /tmp/lzw_body_check && /tmp/lzw_body_check
//
// The emitter below replays what the wave does: 64 "lanes" read their source bytes, then all write - so the KwKwK case and strings
// longer than a wave go through the same index arithmetic as on the device. Source and destination buffers are heap blocks of exactly
// the stated size, so any access outside them stops the program. Inputs:
//   1. the random byte strings and capacities of tests/test_tiff_io.py::test_decoders_and_reader_survive_random_corruption (10 000);
//   2. valid streams (noise, constant, periodic, smooth, with and without EOI) from a small encoder, decoded with exact, short and
//      over-long capacities;
//   3. those streams damaged as that test damages its files: 1..20 random bytes overwritten, one in five truncated (30 000).
// Every result is compared with hm_tiff_lzw_decode: same return value, and the same bytes where it is not negative.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "hdrmerge.h"
#include "hm_tiff_lzw_body.h"

namespace {

struct LaneReplay {
    uint8_t* out;
    void literal(int64_t op, uint8_t b) { out[op] = b; }
    void copy(int64_t op, uint32_t from, uint32_t n, uint32_t period) {
        for (uint32_t k0 = 0; k0 < n; k0 += 64) {
            uint8_t tmp[64];
            const uint32_t m = n - k0 < 64 ? n - k0 : 64;
            for (uint32_t l = 0; l < m; ++l) { const uint32_t k = k0 + l; tmp[l] = out[from + (k < period ? k : k - period)]; }
            for (uint32_t l = 0; l < m; ++l) out[op + k0 + l] = tmp[l];
        }
    }
};

// TIFF LZW encoder (early change, Clear when the table is full), table as a 4096 x 256 child map
std::vector<uint8_t> encode(const std::vector<uint8_t>& data, bool eoi) {
    std::vector<uint8_t> out;
    uint32_t acc = 0; int have = 0, nbits = 9, next = 258;
    std::vector<int16_t> child(4096 * 256, -1);
    auto put = [&](int code) {
        acc = (acc << nbits) | static_cast<uint32_t>(code); have += nbits;
        while (have >= 8) { out.push_back(static_cast<uint8_t>(acc >> (have - 8))); have -= 8; }
    };
    put(256);
    int cur = -1;
    for (uint8_t b : data) {
        if (cur < 0) { cur = b; continue; }
        const int16_t nx = child[cur * 256 + b];
        if (nx >= 0) { cur = nx; continue; }
        put(cur);
        child[cur * 256 + b] = static_cast<int16_t>(next++);
        if (next >= (1 << nbits) && nbits < 12) ++nbits;           // early change: the decoder's table is one entry behind
        if (next >= 4094) {
            put(256);
            std::fill(child.begin(), child.end(), static_cast<int16_t>(-1));
            next = 258; nbits = 9;
        }
        cur = b;
    }
    if (cur >= 0) {
        put(cur);
        ++next;
        if (next >= (1 << nbits) && nbits < 12) ++nbits;
    }
    if (eoi) put(257);
    if (have > 0) out.push_back(static_cast<uint8_t>(acc << (8 - have)));
    return out;
}

long n_checked = 0, n_errors = 0, n_ok = 0;

void check(const std::vector<uint8_t>& src, int64_t cap) {
    uint8_t* s = static_cast<uint8_t*>(malloc(src.size() ? src.size() : 1));       // exact-size heap blocks: ASan's red zones are the guard
    if (!src.empty()) memcpy(s, src.data(), src.size());
    uint8_t* a = static_cast<uint8_t*>(malloc(cap ? cap : 1));
    uint8_t* b = static_cast<uint8_t*>(malloc(cap ? cap : 1));
    hm_lzw::Table* t = static_cast<hm_lzw::Table*>(malloc(sizeof(hm_lzw::Table)));
    LaneReplay emit{b};
    const int64_t ra = hm_tiff_lzw_decode(s, static_cast<int64_t>(src.size()), a, cap);
    const int64_t rb = hm_lzw::decode(s, static_cast<int64_t>(src.size()), cap, *t, emit);
    if (ra != rb || (ra > 0 && memcmp(a, b, static_cast<size_t>(ra)) != 0)) {
        fprintf(stderr, "MISMATCH: src_len %zu cap %lld host %lld body %lld\n", src.size(), (long long)cap, (long long)ra, (long long)rb);
        exit(1);
    }
    ++n_checked; (ra < 0 ? n_errors : n_ok)++;
    free(s); free(a); free(b); free(t);
}

}  // namespace

int main() {
    std::mt19937 rng(5);
    auto pick = [&](std::initializer_list<int> v) { return *(v.begin() + rng() % v.size()); };
    for (int i = 0; i < 10000; ++i) {                                  // 1. random strings
        const int n = pick({0, 1, 2, 3, 8, 64, 300, 5000});
        std::vector<uint8_t> src(n);
        if (rng() % 10 < 7) for (auto& x : src) x = static_cast<uint8_t>(rng());
        else std::fill(src.begin(), src.end(), static_cast<uint8_t>(pick({0x80, 0x00, 0xff, 0x01})));
        check(src, pick({0, 1, 7, 64, 1000, 70000}));
    }
    std::vector<std::vector<uint8_t>> plain;                           // 2. valid streams
    for (int n : {1, 2, 7, 63, 64, 65, 300, 4096, 12288, 20000}) {
        std::vector<uint8_t> noise(n), constant(n, 0x5a), periodic(n), smooth(n);
        for (int k = 0; k < n; ++k) {
            noise[k] = static_cast<uint8_t>(rng());
            periodic[k] = (k & 1) ? 'B' : 'A';
            smooth[k] = static_cast<uint8_t>(128 + 100 * ((k % 512) / 512.0) + rng() % 2);
        }
        plain.push_back(noise); plain.push_back(constant); plain.push_back(periodic); plain.push_back(smooth);
    }
    std::vector<std::vector<uint8_t>> streams;
    for (const auto& p : plain)
        for (bool eoi : {true, false}) {
            streams.push_back(encode(p, eoi));
            const int64_t n = static_cast<int64_t>(p.size());
            std::vector<uint8_t> back(n);
            if (hm_tiff_lzw_decode(streams.back().data(), static_cast<int64_t>(streams.back().size()), back.data(), n) != n || back != p) {
                fprintf(stderr, "the encoder's stream does not decode to its input (n = %lld)\n", (long long)n);
                return 1;
            }
            for (int64_t cap : {n, n - 1, n / 2, n + 1, n + 100, int64_t{0}}) check(streams.back(), cap < 0 ? 0 : cap);
        }
    for (int i = 0; i < 30000; ++i) {                                  // 3. damaged streams
        const auto& base = streams[rng() % streams.size()];
        std::vector<uint8_t> b = base;
        const int hits = pick({1, 1, 2, 5, 20});
        for (int k = 0; k < hits; ++k) {
            const size_t lim = (rng() % 10 < 7 && b.size() > 400) ? 400 : b.size();
            b[rng() % lim] = static_cast<uint8_t>(rng());
        }
        if (rng() % 5 == 0) b.resize(rng() % b.size());
        check(b, pick({0, 1, 7, 64, 1000, 12288, 70000}));
    }
    printf("lzw body check: %ld streams, %ld decoded, %ld refused, all equal to hm_tiff_lzw_decode\n", n_checked, n_ok, n_errors);
    return 0;
}
