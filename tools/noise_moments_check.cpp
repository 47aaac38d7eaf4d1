// noise_moments_check.cpp - a stand-alone program on the HOST build's noise-moments entry points (hm_noise_moments_update_u16,
// hm_noise_moments_std, hm_noise_moments_update_u16_describe, hm_noise_moments_algorithmic_bytes), made to be compiled together with
// csrc_host/hm_host.cpp under -fsanitize=address,undefined and run once:
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude \
//       -Icamera_linearity_amd/csrc tools/noise_moments_check.cpp camera_linearity_amd/csrc_host/hm_host.cpp -o noise_moments_check
//
// The cases are those of tests/test_noise_moments_host.py: C = 1..4, depths 9, 10, 11, 12 and 16, 1, 2, 31 and 32 frames, shape (7, 13, C),
// frames and mean at a 2-byte offset in buffers that end with the last element (a read past it is a heap overflow), bits set above the
// depth, a constant mean frame, two launches into one state; then the table on the exact-oracle rows (n = 0, N = 0, d = +-M at 16 bits,
// counts of 2^40) and every refusal of the rules with nothing written. Every result is compared with a plain restatement. Exit status 0
// and "noise_moments_check: ok" when everything holds.
#include "hdrmerge.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static void restate(const std::vector<const uint16_t*>& frames, const uint16_t* mean, int64_t n, int C, int depth, std::vector<int64_t>& mom) {
    const uint32_t M = (1u << depth) - 1u;
    for (const uint16_t* f : frames)
        for (int64_t e = 0; e < n; ++e) {
            const int64_t m = mean[e] & M, d = static_cast<int64_t>(f[e] & M) - m;
            int64_t* t = mom.data() + (m * C + e % C) * 3;
            t[0] += 1; t[1] += d; t[2] += d * d;
        }
}

static void moments_cases() {
    std::mt19937_64 rng(7);
    const int depths[] = {9, 10, 11, 12, 16}, counts[] = {1, 2, 31, 32};
    for (int C = 1; C <= 4; ++C)
        for (int depth : depths)
            for (int N : counts) {
                const int64_t n = 7 * 13 * C;
                const uint32_t M = (1u << depth) - 1u;
                // exactly sized buffers, one spare element in front: the views start 2 bytes in and end with the allocation
                std::vector<std::vector<uint16_t>> bufs(N, std::vector<uint16_t>(n + 1));
                std::vector<uint16_t> mean_buf(n + 1), const_mean(n);
                std::vector<const uint16_t*> views;
                std::vector<const void*> ptrs;
                for (auto& b : bufs) {
                    for (auto& v : b) v = static_cast<uint16_t>(rng());           // every bit, also above the depth
                    views.push_back(b.data() + 1);
                    ptrs.push_back(b.data() + 1);
                }
                for (auto& v : mean_buf) v = static_cast<uint16_t>(rng());
                bufs[0][1] = 0; mean_buf[1] = static_cast<uint16_t>(M);            // d = -M
                if (n > 1) { bufs[0][2] = static_cast<uint16_t>(M); mean_buf[2] = 0; }    // d = +M
                const uint16_t* mean = mean_buf.data() + 1;
                const size_t rows = static_cast<size_t>(1) << depth;
                for (int variant = 0; variant <= 3; ++variant) {
                    if (variant == 1 && int64_t{20} * static_cast<int64_t>(rows) * C > 128 * 1024) continue;
                    std::vector<int64_t> got(rows * C * 3, 0), want(rows * C * 3, 0);
                    CHECK(hm_noise_moments_update_u16(ptrs.data(), N, mean, n, C, depth, got.data(), variant, nullptr) == HM_OK);
                    restate(views, mean, n, C, depth, want);
                    CHECK(got == want);
                    // a second launch into the same state
                    CHECK(hm_noise_moments_update_u16(ptrs.data(), N > 1 ? N - 1 : 1, mean, n, C, depth, got.data(), variant, nullptr) == HM_OK);
                    restate(std::vector<const uint16_t*>(views.begin(), views.begin() + (N > 1 ? N - 1 : 1)), mean, n, C, depth, want);
                    CHECK(got == want);
                }
                for (auto& v : const_mean) v = static_cast<uint16_t>(mean[0]);
                std::vector<int64_t> got(rows * C * 3, 0), want(rows * C * 3, 0);
                CHECK(hm_noise_moments_update_u16(ptrs.data(), N, const_mean.data(), n, C, depth, got.data(), 0, nullptr) == HM_OK);
                restate(views, const_mean.data(), n, C, depth, want);
                CHECK(got == want);
                std::vector<double> table(rows * C);
                CHECK(hm_noise_moments_std(got.data(), C, depth, table.data(), nullptr) == HM_OK);
                for (size_t i = 0; i < rows * C; ++i) CHECK((got[i * 3] == 0) == std::isnan(table[i]));
            }
}

static void table_cases() {
    const int depth = 16, C = 4;
    const int64_t M = 65535;
    const size_t rows = 65536;
    std::vector<int64_t> mom(rows * C * 3, 0);
    std::vector<double> out(rows * C, -1.0);
    struct Row { int64_t n, s1, s2; double want; };
    const int64_t big = int64_t{1} << 40;
    const Row cases[] = {{0, 0, 0, NAN}, {5, 15, 45, 0.0}, {1, -M, M * M, 0.0}, {big, big, big, 0.0},
                         {2, 0, 2 * M * M, 1.0},                              // d = +M, -M: std = M / M
                         {big, 0, big, 1.0 / 65535.0},                        // half at +1, half at -1
                         {big, 0, big * 181 * 181, 181.0 / 65535.0},
                         {4, 0, 4 * 100 * 100, 100.0 / 65535.0}};
    size_t slot = 5;
    for (const Row& r : cases) {
        mom[slot * 3] = r.n; mom[slot * 3 + 1] = r.s1; mom[slot * 3 + 2] = r.s2;
        slot += 4099;
    }
    CHECK(hm_noise_moments_std(mom.data(), C, depth, out.data(), nullptr) == HM_OK);
    slot = 5;
    for (const Row& r : cases) {
        const double got = out[slot];
        if (std::isnan(r.want)) CHECK(std::isnan(got));
        else if (r.want == 0.0) CHECK(got == 0.0 && !std::signbit(got));
        else CHECK(std::fabs(got - r.want) <= 8 * 0x1.0p-53 * r.want);
        slot += 4099;
    }
    size_t nans = 0;
    for (double v : out) nans += std::isnan(v);
    CHECK(nans == rows * C - (sizeof(cases) / sizeof(cases[0]) - 1));
}

static void rule_cases() {
    uint16_t frame[16] = {}, mean[16] = {};
    std::vector<int64_t> mom(2048 * 3 * 3, 0);
    const void* ptrs[2] = {frame, frame};
    const void* odd[2] = {frame, reinterpret_cast<const char*>(frame) + 1};
    const void* holed[2] = {frame, nullptr};
    CHECK(hm_noise_moments_update_u16(ptrs, 33, mean, 12, 3, 11, mom.data(), 0, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_update_u16(ptrs, 2, mean, 12, 3, 8, mom.data(), 0, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_update_u16(ptrs, 2, mean, 12, 3, 17, mom.data(), 0, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_update_u16(ptrs, 2, mean, 12, 3, 11, mom.data(), 4, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_update_u16(ptrs, 2, mean, 12, 5, 11, mom.data(), 0, nullptr) == HM_EUNSUPPORTED);
    CHECK(hm_noise_moments_update_u16(ptrs, 2, mean, 11, 3, 11, mom.data(), 0, nullptr) == HM_ESHAPE);
    CHECK(hm_noise_moments_update_u16(ptrs, 2, mean, 12, 3, 12, mom.data(), 1, nullptr) == HM_EUNSUPPORTED);
    CHECK(hm_noise_moments_update_u16(nullptr, 2, mean, 12, 3, 11, mom.data(), 0, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_update_u16(ptrs, 2, nullptr, 12, 3, 11, mom.data(), 0, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_update_u16(ptrs, 2, mean, 12, 3, 11, nullptr, 0, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_update_u16(holed, 2, mean, 12, 3, 11, mom.data(), 0, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_update_u16(odd, 2, mean, 12, 3, 11, mom.data(), 0, nullptr) == HM_EALIGN);
    CHECK(hm_noise_moments_update_u16(ptrs, 2, reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(mean) + 1), 12, 3, 11, mom.data(), 0,
                                      nullptr) == HM_EALIGN);
    CHECK(hm_noise_moments_update_u16(ptrs, 0, mean, 12, 3, 11, mom.data(), 0, nullptr) == HM_OK);
    CHECK(hm_noise_moments_update_u16(ptrs, 2, mean, 0, 3, 11, mom.data(), 0, nullptr) == HM_OK);
    for (int64_t v : mom) CHECK(v == 0);
    double out[4];
    CHECK(hm_noise_moments_std(nullptr, 3, 11, out, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_std(mom.data(), 3, 11, nullptr, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_std(mom.data(), 3, 8, out, nullptr) == HM_EINVAL);
    CHECK(hm_noise_moments_std(mom.data(), 5, 11, out, nullptr) == HM_EUNSUPPORTED);
    char name[8];                                                             // shorter than the name: it is cut, not overrun
    CHECK(hm_noise_moments_update_u16_describe(12, 2, 3, 11, 0, name, sizeof name) == HM_OK && std::strlen(name) == 7);
    CHECK(hm_noise_moments_update_u16_describe(12, 2, 3, 11, 0, nullptr, 8) == HM_EINVAL);
    CHECK(hm_noise_moments_update_u16_describe(12, 2, 3, 12, 1, name, sizeof name) == HM_EUNSUPPORTED && name[0] == '\0');
    CHECK(hm_noise_moments_algorithmic_bytes(32, 1000, 4, 16) == 2 * 1000 * 33 + int64_t{2} * 24 * 65536 * 4);
}

int main() {
    moments_cases();
    table_cases();
    rule_cases();
    if (failures) {
        std::printf("noise_moments_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("noise_moments_check: ok\n");
    return 0;
}
