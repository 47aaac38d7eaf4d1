// lzw_enc_body_check.cpp - host check of the device LZW encoder's body (camera_linearity_amd/csrc/hm_tiff_lzw_enc_body.h) under
// AddressSanitizer / UBSan, before the kernel that runs it sees a GPU. A development step for whoever changes that header: a stand-alone
// program, not part of the library, the package or the test suite, and it needs no GPU.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icamera_linearity_amd/csrc \
//       tools/lzw_enc_body_check.cpp -o /tmp/lzw_enc_body_check && /tmp/lzw_enc_body_check
//
// The ops below replay what the wave of hm_tiff_encode.hip does, serially: the input arrives as 64 aligned dwords per 256-byte chunk
// (with the chunk behind it fetched ahead, and no dword read at or past the strip's length), a probe reads 64 consecutive slots, builds
// the two ballots and takes the first hit that lies before the first free slot, a Clear empties the table 16 bytes per "lane", and
// output words wait in 64 "registers" that leave together. Input, output and dictionary are heap blocks of exactly the sizes the
// library gives them (round_up(n, 16), round_up(bound(n), 16), sizeof(Dict)), so any access outside them stops the program.
// Every stream is checked three ways: it is within bound(n); it equals the stream of the body's own serial ops; and the decoder body
// (hm_tiff_lzw_body.h) returns the input from it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "hm_tiff_lzw_body.h"
#include "hm_tiff_lzw_enc_body.h"

namespace {

using hm_lzw_enc::Dict;
using hm_lzw_enc::kSlots;

struct WaveReplay {
    int64_t n;
    int64_t chunk = -1;
    uint32_t cur[64] = {}, ahead[64] = {}, mine[64] = {};
    long probes = 0, windows_past_first = 0, clears = 0;

    void load(const uint8_t* src, int64_t c, uint32_t* dst) const {
        for (int lane = 0; lane < 64; ++lane) {
            const int64_t at = c * 256 + lane * 4;
            dst[lane] = 0;
            if (at < n) memcpy(&dst[lane], src + at, 4);            // an aligned dword: may reach round_up(n, 4), inside the slot
        }
    }
    uint8_t byte(const uint8_t* src, int64_t i) {
        const int64_t c = i >> 8;
        if (c != chunk) {
            if (chunk >= 0 && c == chunk + 1) memcpy(cur, ahead, sizeof cur);
            else load(src, c, cur);
            load(src, c + 1, ahead);
            chunk = c;
        }
        return static_cast<uint8_t>(cur[(i >> 2) & 63] >> ((i & 3) * 8));
    }
    void clear(Dict& d) {
        ++clears;
        for (int lane = 0; lane < 64; ++lane)
            for (int k = lane; k < kSlots / 4; k += 64) memset(&d.slot[4 * k], 0, 16);
    }
    int probe(const Dict& d, uint32_t start, uint32_t key, uint32_t* free_slot) {
        uint32_t e[64];
        uint64_t hit = 0, empty = 0;
        for (int lane = 0; lane < 64; ++lane) {
            e[lane] = d.slot[(start + lane) & (kSlots - 1)];
            if (e[lane] != 0 && (e[lane] >> 12) == key) hit |= 1ull << lane;
            if (e[lane] == 0) empty |= 1ull << lane;
        }
        ++probes;
        const int first_hit = hit ? __builtin_ctzll(hit) : 64, first_empty = empty ? __builtin_ctzll(empty) : 64;
        if (first_hit < first_empty) return static_cast<int>(e[first_hit] & 0xFFFu);
        if (first_empty < 64) { *free_slot = (start + first_empty) & (kSlots - 1); return -1; }
        ++windows_past_first;
        return -2;
    }
    void insert(Dict& d, uint32_t slot, uint32_t word) { d.slot[slot] = word; }
    void word(uint8_t* out, int64_t w, uint32_t v) {
        const int k = static_cast<int>(w & 63);
        mine[k] = v;
        if (k == 63) for (int lane = 0; lane < 64; ++lane) memcpy(out + 4 * (w - 63 + lane), &mine[lane], 4);
    }
    void flush(uint8_t* out, int64_t n_words) {
        const int k = static_cast<int>(n_words & 63);
        for (int lane = 0; lane < k; ++lane) memcpy(out + 4 * (n_words - k + lane), &mine[lane], 4);
    }
};

struct SerialEmit {
    uint8_t* out;
    void literal(int64_t op, uint8_t b) { out[op] = b; }
    void copy(int64_t op, uint32_t from, uint32_t n, uint32_t period) {
        for (uint32_t k = 0; k < n; ++k) out[op + k] = out[from + (k < period ? k : k - period)];
    }
};

int64_t round16(int64_t x) { return (x + 15) & ~int64_t{15}; }

long n_streams = 0, n_clears = 0, n_probes = 0, n_second_windows = 0;
int64_t in_bytes = 0, out_bytes = 0;
double worst_ratio = 0;

void check(const std::vector<uint8_t>& data) {
    const int64_t n = static_cast<int64_t>(data.size()), cap = hm_lzw_enc::bound(n);
    uint8_t* src = static_cast<uint8_t*>(aligned_alloc(16, static_cast<size_t>(round16(n ? n : 1))));   // exact-size heap blocks: ASan's red zones are the guard
    if (n) memcpy(src, data.data(), static_cast<size_t>(n));
    uint8_t* a = static_cast<uint8_t*>(aligned_alloc(16, static_cast<size_t>(round16(cap))));
    uint8_t* b = static_cast<uint8_t*>(aligned_alloc(16, static_cast<size_t>(round16(cap))));
    Dict* d = static_cast<Dict*>(malloc(sizeof(Dict)));
    WaveReplay wave;
    wave.n = n;
    hm_lzw_enc::SerialOps serial;
    const int64_t ra = hm_lzw_enc::encode(src, n, a, cap, *d, wave);
    const int64_t rb = hm_lzw_enc::encode(src, n, b, cap, *d, serial);
    if (ra <= 0 || ra > cap || ra != rb || memcmp(a, b, static_cast<size_t>(ra)) != 0) {
        fprintf(stderr, "MISMATCH: n %lld bound %lld wave %lld serial %lld\n", (long long)n, (long long)cap, (long long)ra, (long long)rb);
        exit(1);
    }
    uint8_t* back = static_cast<uint8_t*>(malloc(static_cast<size_t>(n ? n : 1)));
    hm_lzw::Table* t = static_cast<hm_lzw::Table*>(malloc(sizeof(hm_lzw::Table)));
    SerialEmit emit{back};
    const int64_t rd = hm_lzw::decode(a, ra, n, *t, emit);
    if (rd != n || (n && memcmp(back, data.data(), static_cast<size_t>(n)) != 0)) {
        fprintf(stderr, "the decoder body does not return the input: n %lld decoded %lld\n", (long long)n, (long long)rd);
        exit(1);
    }
    if (n >= 64 && static_cast<double>(ra) / cap > worst_ratio) worst_ratio = static_cast<double>(ra) / cap;
    ++n_streams; n_clears += wave.clears - 1; n_probes += wave.probes; n_second_windows += wave.windows_past_first;
    in_bytes += n; out_bytes += ra;
    free(src); free(a); free(b); free(d); free(back); free(t);
}

// The continuation of a lookup past its first window, which no stream above reaches (random hashing keeps runs of used slots short):
// runs of 63 .. 200 used slots are laid by hand behind a key's start - also across the end of the table - and hm_lzw_enc::find must
// report the slot behind the run as free, and after the insert return the code from there, with the wave replay and the serial ops alike.
long n_directed = 0, n_directed_windows = 0;

void check_long_runs() {
    Dict* d = static_cast<Dict*>(malloc(sizeof(Dict)));
    std::vector<uint32_t> keys = {0u, 0x41u << 8 | 0x42u, 4093u << 8 | 255u};
    for (uint32_t k = 1; k < (1u << 20) && keys.size() < 6; ++k)
        if (hm_lzw_enc::start_of(k) > kSlots - 40) keys.push_back(k);              // the run wraps round the end of the table
    for (uint32_t key : keys)
        for (uint32_t run : {0u, 1u, 63u, 64u, 65u, 127u, 128u, 129u, 200u}) {
            const uint32_t s0 = hm_lzw_enc::start_of(key), behind = (s0 + run) & (kSlots - 1);
            hm_lzw_enc::SerialOps serial;
            WaveReplay wave;
            wave.n = 0;
            serial.clear(*d);
            for (uint32_t j = 0; j < run; ++j) d->slot[(s0 + j) & (kSlots - 1)] = (((key + 1 + j) & 0xFFFFFu) << 12) | 300u;   // other keys
            uint32_t fa = ~0u, fb = ~0u;
            const int ra = hm_lzw_enc::find(*d, key, wave, &fa), rb = hm_lzw_enc::find(*d, key, serial, &fb);
            if (ra != -1 || rb != -1 || fa != behind || fb != behind) {
                fprintf(stderr, "long run: key %u run %u: wave %d slot %u, serial %d slot %u, expected free slot %u\n", key, run, ra, fa, rb, fb, behind);
                exit(1);
            }
            wave.insert(*d, fa, (key << 12) | 1234u);
            const int ha = hm_lzw_enc::find(*d, key, wave, &fa), hb = hm_lzw_enc::find(*d, key, serial, &fb);
            if (ha != 1234 || hb != 1234) {
                fprintf(stderr, "long run: key %u run %u: inserted code not found (wave %d, serial %d)\n", key, run, ha, hb);
                exit(1);
            }
            n_directed += 2; n_directed_windows += wave.windows_past_first;
        }
    for (int k = 0; k < kSlots; ++k) d->slot[k] = (0xFFFFFu << 12) | 300u;         // a full table of another key: every window, then -2
    hm_lzw_enc::SerialOps serial;
    WaveReplay wave;
    uint32_t f = 0;
    if (hm_lzw_enc::find(*d, 5u, wave, &f) != -2 || hm_lzw_enc::find(*d, 5u, serial, &f) != -2 || wave.probes != kSlots / 64) {
        fprintf(stderr, "full table: the lookup did not end with -2 after %d windows\n", kSlots / 64);
        exit(1);
    }
    free(d);
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    check_long_runs();
    std::vector<int64_t> sizes = {0, 1, 2, 3, 255, 256};
    for (int64_t n = 3835; n <= 3840; ++n) sizes.push_back(n);
    for (int64_t n = 4093; n <= 4096; ++n) sizes.push_back(n);
    for (int64_t n : {8192, 8193, 12288, 16383, 16384, 16385, 24576, 32768, 49152, 65535, 65536, 98303, 98304}) sizes.push_back(n);
    for (int64_t n : sizes) {
        std::vector<uint8_t> zeros(n, 0), ramp(n), noise(n), pairs(n);
        for (int64_t k = 0; k < n; ++k) {
            ramp[k] = static_cast<uint8_t>(k);
            noise[k] = static_cast<uint8_t>(rng());
            pairs[k] = static_cast<uint8_t>((k % 256) * (k / 256 + 1));                 // stride k / 256 + 1: pairs (a, a + stride) are new
        }
        check(zeros); check(ramp); check(noise); check(pairs);
    }
    const long fixed = n_streams;
    for (int i = 0; i < 4000; ++i) {                                   // random strings of random alphabets
        const int alphabet = 1 + static_cast<int>(rng() % (i % 3 == 0 ? 3 : 256));
        const int64_t n = i % 50 == 0 ? 20000 + rng() % 40000 : rng() % 6000;
        std::vector<uint8_t> data(n);
        const uint8_t base = static_cast<uint8_t>(rng());
        for (auto& x : data) x = static_cast<uint8_t>(base + rng() % alphabet);
        check(data);
    }
    printf("lzw encoder body check: %ld streams (%ld of fixed sizes and kinds, %ld random), %lld bytes in, %lld out, %ld Clears after the first,\n"
           "%ld probes of 64 slots of which %ld went on to a further window; worst size / bound %.3f; every stream within the bound, equal to\n"
           "the serial ops' stream, and decoded back to its input by the decoder body; %ld directed lookups behind hand-laid runs of up to 200\n"
           "used slots (%ld continuations into a further window) and a full table ended where they must\n",
           n_streams, fixed, n_streams - fixed, (long long)in_bytes, (long long)out_bytes, n_clears, n_probes, n_second_windows, worst_ratio,
           n_directed, n_directed_windows);
    return 0;
}
