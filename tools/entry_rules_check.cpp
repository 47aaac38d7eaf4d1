// entry_rules_check.cpp - the shared argument rules of the TIFF, calibration, producer, all-pairs, linearize, operator and pointwise
// entries (camera_linearity_amd/csrc/hm_tiff_rules.h, hm_calibration_rules.h, hm_producer_rules.h, hm_pairs_rules.h, hm_frame_rules.h,
// hm_ops_rules.h on hm_rules_common.h) under AddressSanitizer / UBSan: every per-frame, per-problem,
// per-pair, index, shape and stride array is a heap block of EXACTLY the count passed, at the smallest and the largest counts, the NULL
// cases, and extents at INT_MAX / 2^62 - a rule that reads one entry too many, looks through a pointer it was to refuse, or forms a
// product that overflows stops the program.
// A development step for whoever changes those headers: a stand-alone program, not part of the library, the package or the test suite,
// and it needs no GPU.
//
// Build and run (one command line):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icamera_linearity_amd/csrc
//       tools/entry_rules_check.cpp -o /tmp/entry_rules_check && /tmp/entry_rules_check
#include <cstdio>
#include <limits>
#include <vector>
#include "hm_calibration_rules.h"
#include "hm_frame_rules.h"
#include "hm_ops_rules.h"
#include "hm_pairs_rules.h"
#include "hm_producer_rules.h"
#include "hm_tiff_rules.h"

namespace {

int failures = 0;
void expect(const char* what, long long got, long long want) {
    if (got != want) { std::printf("FAIL %s: %lld, expected %lld\n", what, got, want); ++failures; }
}

// addresses that are never read: the rules look at pointers, not through them (only the per-frame / per-problem / per-pair arrays are read)
template <class T> T* fake(uintptr_t a) { return reinterpret_cast<T*>(a); }
const double kNaN = std::numeric_limits<double>::quiet_NaN();

void producers() {
    using namespace hm_rules;
    bool empty;
    double* mean = fake<double>(0x1000);
    for (int n : {1, 2, HM_MAX_FRAMES}) {
        std::vector<const void*> frames(n, fake<void>(0x2000));
        expect("welford", check_welford_update(frames.data(), n, 0, mean, 12, 3, empty), HM_OK);
        expect("welford, at the count limit", check_welford_update(frames.data(), n, kWelfordMaxCount, mean, 12, 3, empty), HM_OK);
        expect("welford, beyond it", check_welford_update(frames.data(), n, kWelfordMaxCount + 1, mean, 12, 3, empty), HM_EUNSUPPORTED);
        expect("welford, too many frames", check_welford_update(frames.data(), HM_MAX_FRAMES + 1, 0, mean, 12, 3, empty), HM_EINVAL);
        expect("welford, negative frames", check_welford_update(frames.data(), -1, 0, mean, 12, 3, empty), HM_EINVAL);
        expect("noise", check_noise_profile_update(frames.data(), n, fake<uint8_t>(0x3000), 12, 3, fake<int64_t>(0x4000), 0, empty), HM_OK);
        expect("noise, too many frames",
               check_noise_profile_update(frames.data(), HM_MAX_FRAMES + 1, fake<uint8_t>(0x3000), 12, 3, fake<int64_t>(0x4000), 0, empty), HM_EINVAL);
        expect("welford u16", check_welford_update_u16(frames.data(), n, 0, nullptr, mean, 12, 3, 12, 0, empty), HM_OK);
        expect("welford u16, too many frames", check_welford_update_u16(frames.data(), HM_MAX_FRAMES + 1, 0, nullptr, mean, 12, 3, 12, 0, empty), HM_EINVAL);
        expect("welford u16, 17 bits", check_welford_update_u16(frames.data(), n, 0, nullptr, mean, 12, 3, 17, 0, empty), HM_EINVAL);
        expect("welford u16, global without a table", check_welford_update_u16(frames.data(), n, 0, nullptr, mean, 12, 3, 12, WELFORD_U16_GLOBAL, empty), HM_EUNSUPPORTED);
        expect("welford u16, computed with a table", check_welford_update_u16(frames.data(), n, 0, mean, mean, 12, 3, 12, WELFORD_U16_COMPUTED, empty), HM_EUNSUPPORTED);
        expect("welford u16, LDS at 16 bits", check_welford_update_u16(frames.data(), n, 0, nullptr, mean, 12, 3, 16, WELFORD_U16_LDS, empty), HM_EUNSUPPORTED);
        expect("welford u16, LDS, C = 3 at 13 bits", check_welford_update_u16(frames.data(), n, 0, mean, mean, 12, 3, 13, WELFORD_U16_LDS, empty), HM_EUNSUPPORTED);
        expect("welford u16, LDS, C = 3 at 12 bits", check_welford_update_u16(frames.data(), n, 0, mean, mean, 12, 3, 12, WELFORD_U16_LDS, empty), HM_OK);
        frames[n - 1] = fake<void>(0x2001);
        expect("welford u16, last frame odd", check_welford_update_u16(frames.data(), n, 0, nullptr, mean, 12, 3, 12, 0, empty), HM_EALIGN);
        frames[n - 1] = nullptr;
        expect("welford u16, last frame NULL", check_welford_update_u16(frames.data(), n, 0, nullptr, mean, 12, 3, 12, 0, empty), HM_EINVAL);
        expect("welford, last frame NULL", check_welford_update(frames.data(), n, 0, mean, 12, 3, empty), HM_EINVAL);
        expect("noise, last frame NULL", check_noise_profile_update(frames.data(), n, fake<uint8_t>(0x3000), 12, 3, fake<int64_t>(0x4000), 0, empty), HM_EINVAL);
    }
    expect("welford, no frames", check_welford_update(nullptr, 0, 0, nullptr, 12, 3, empty), HM_OK);
    expect("welford, no frames: empty", empty, 1);
    expect("welford, frames NULL", check_welford_update(nullptr, 2, 0, mean, 12, 3, empty), HM_EINVAL);
    expect("welford, C = 0", check_welford_update(nullptr, 2, 0, mean, 12, 0, empty), HM_ESHAPE);
    expect("noise, C = 0", check_noise_profile_update(nullptr, 2, nullptr, 12, 0, nullptr, 0, empty), HM_EINVAL);
    expect("noise, frames NULL", check_noise_profile_update(nullptr, 2, fake<uint8_t>(0x3000), 12, 3, fake<int64_t>(0x4000), 0, empty), HM_EINVAL);
    expect("finalize", check_welford_finalize(mean, mean, 2, fake<uint8_t>(0x5000), fake<uint8_t>(0x6000), 12, empty), HM_OK);
    expect("finalize, all NULL", check_welford_finalize(nullptr, nullptr, 1, nullptr, nullptr, 12, empty), HM_OK);
    expect("finalize, one frame", check_welford_finalize(mean, mean, 1, nullptr, fake<uint8_t>(0x6000), 12, empty), HM_EINVAL);
    expect("welford u16, no frames", check_welford_update_u16(nullptr, 0, 0, nullptr, nullptr, 12, 3, 12, WELFORD_U16_GLOBAL, empty), HM_OK);
    expect("welford u16, no frames: empty", empty, 1);
    expect("welford u16, frames NULL", check_welford_update_u16(nullptr, 2, 0, nullptr, mean, 12, 3, 12, 0, empty), HM_EINVAL);
    for (int bits = 9; bits <= 16; ++bits)
        for (int C = 1; C <= HM_MAX_CHANNELS; ++C) {
            expect("welford u16, fit rule with a table", welford_u16_table_fits_lds(bits, C, true), bits <= (C == 1 ? 14 : C == 2 ? 13 : 12));
            expect("welford u16, fit rule without one", welford_u16_table_fits_lds(bits, C, false), bits <= 14);
            for (bool with_icrf : {false, true})
                expect("welford u16, the default applies", welford_u16_placement_applies(welford_u16_default_placement(bits, C, with_icrf), bits, C, with_icrf), 1);
        }
    expect("finalize u16", check_welford_finalize_u16(mean, mean, 2, 12, fake<uint16_t>(0x5000), fake<uint16_t>(0x6000), 12, empty), HM_OK);
    expect("finalize u16, all NULL", check_welford_finalize_u16(nullptr, nullptr, 1, 12, nullptr, nullptr, 12, empty), HM_OK);
    expect("finalize u16, 8 bits", check_welford_finalize_u16(mean, mean, 2, 8, fake<uint16_t>(0x5000), fake<uint16_t>(0x6000), 12, empty), HM_EINVAL);
    expect("finalize u16, one frame", check_welford_finalize_u16(mean, mean, 1, 12, nullptr, fake<uint16_t>(0x6000), 12, empty), HM_EINVAL);
    expect("finalize u16, odd output", check_welford_finalize_u16(mean, mean, 2, 12, fake<uint16_t>(0x5001), nullptr, 12, empty), HM_EALIGN);
    expect("welford, the shared counts: the count limit before the shape", welford_update_counts(2, kWelfordMaxCount + 1, 12, 0, empty), HM_EUNSUPPORTED);
    expect("welford, the shared pointers: frames NULL, none read", welford_update_pointers(nullptr, HM_MAX_FRAMES, mean), HM_EINVAL);
    expect("welford u16, a depth rule broken before the count limit", check_welford_update_u16_counts(2, kWelfordMaxCount + 1, 12, 3, false, 8, 0, empty), HM_EINVAL);
    expect("finalize u16, a depth rule broken before nothing to do", check_welford_finalize_u16(nullptr, nullptr, 1, 17, nullptr, nullptr, 0, empty), HM_EINVAL);
    expect("welford bytes, uint8 frames with m2", welford_algorithmic_bytes(1, HM_MAX_FRAMES, true, 10), 10 * (HM_MAX_FRAMES + 32));
    expect("welford bytes, uint16 frames without", welford_algorithmic_bytes(2, HM_MAX_FRAMES, false, 10), 10 * (2 * HM_MAX_FRAMES + 16));
    expect("welford bytes, 2^40 elements", welford_algorithmic_bytes(2, HM_MAX_FRAMES, true, int64_t{1} << 40), (int64_t{1} << 40) * 96);   // no int overflow
    expect("noise std, NULL", check_noise_profile_std(nullptr, 3, nullptr, nullptr), HM_EINVAL);
    expect("noise std, 5 channels", check_noise_profile_std(fake<int64_t>(0x4000), 5, mean, mean), HM_EUNSUPPORTED);
    expect("clean edges, NULL", check_noise_profile_clean_edges(nullptr, 3), HM_EINVAL);
    for (bool need_ws : {false, true}) {
        expect("kde moments", check_kde_moments(mean, 12, 3, 1, mean, mean, 64, need_ws), HM_OK);
        expect("kde moments, C = 0", check_kde_moments(mean, 12, 0, 0, mean, mean, 64, need_ws), HM_EINVAL);             // no division by C = 0
        expect("kde moments, NULL workspace", check_kde_moments(mean, 12, 3, 1, mean, nullptr, 64, need_ws), need_ws ? HM_EINVAL : HM_OK);
        expect("kde moments, NULL moments and a bad shape", check_kde_moments(mean, 11, 3, 1, nullptr, mean, 64, need_ws), need_ws ? HM_ESHAPE : HM_EINVAL);
        expect("kde evaluate", check_kde_evaluate(mean, 12, 3, 1, 0.5, 1.0, mean, 4, mean, mean, 64, need_ws, empty), HM_OK);
        expect("kde evaluate, C = 0", check_kde_evaluate(mean, 12, 0, 0, 0.5, 1.0, mean, 4, mean, mean, 64, need_ws, empty), HM_EINVAL);
        expect("kde evaluate, NaN h", check_kde_evaluate(mean, 12, 3, 1, kNaN, 1.0, mean, 4, mean, mean, 64, need_ws, empty), HM_EINVAL);
        expect("kde evaluate, no points", check_kde_evaluate(mean, 12, 3, 1, 0.5, 1.0, nullptr, 0, nullptr, mean, 64, need_ws, empty), HM_OK);
        expect("kde evaluate, no points: empty", empty, 1);
    }
}

void calibration() {
    using namespace hm_rules;
    bool empty;
    double* d = fake<double>(0x1000);
    uint8_t* b = fake<uint8_t>(0x2000);
    int64_t* s = fake<int64_t>(0x3000);
    expect("energy", check_linearity_energy(b, d, d, 2, 5, 250, 8, 2, d, empty), HM_OK);
    expect("energy, 32 frames, 65535 candidates", check_linearity_energy(b, d, d, kEnergyMaxCandidates, 0, 255, 8, HM_MAX_FRAMES, d, empty), HM_OK);
    expect("energy, 65536 candidates", check_linearity_energy(b, d, d, kEnergyMaxCandidates + 1, 0, 255, 8, 2, d, empty), HM_EUNSUPPORTED);
    expect("energy, no candidates", check_linearity_energy(nullptr, nullptr, nullptr, 0, 0, 255, 8, 2, nullptr, empty), HM_OK);
    expect("energy, no candidates: empty", empty, 1);
    expect("energy, NULL", check_linearity_energy(nullptr, nullptr, nullptr, 2, 0, 255, 8, 2, nullptr, empty), HM_EINVAL);
    uint16_t* w = fake<uint16_t>(0x4000);
    auto e16 = [&](const uint16_t* dn, int cands, int lower, int upper, int frames, int bits, int variant) {
        return check_linearity_energy_u16(dn, d, d, cands, lower, upper, 8, frames, bits, variant, d, empty);
    };
    for (int bits = 9; bits <= 16; ++bits) {
        const int top = (1 << bits) - 1;
        expect("energy u16, limits at the ends", e16(w, 2, 0, top, 2, bits, 0), HM_OK);
        expect("energy u16, upper beyond the depth", e16(w, 2, 0, top + 1, 2, bits, 0), HM_EINVAL);
        expect("energy u16, lower beyond the depth", e16(w, 2, top + 1, top, 2, bits, 2), HM_EINVAL);
        expect("energy u16, row in LDS", e16(w, 2, 0, top, 2, bits, 1), bits <= 14 ? HM_OK : HM_EUNSUPPORTED);
        expect("energy u16, row fits LDS", energy_u16_row_fits_lds(bits), bits <= 14);
    }
    expect("energy u16, 32 frames, 65535 candidates", e16(w, kEnergyMaxCandidates, 5, 4000, HM_MAX_FRAMES, 12, 0), HM_OK);
    expect("energy u16, 65536 candidates", e16(w, kEnergyMaxCandidates + 1, 5, 4000, 2, 12, 0), HM_EUNSUPPORTED);
    expect("energy u16, 8 bits", e16(w, 2, 5, 250, 2, 8, 0), HM_EINVAL);
    expect("energy u16, 17 bits", e16(w, 2, 5, 250, 2, 17, 0), HM_EINVAL);
    expect("energy u16, variant 3", e16(w, 2, 5, 250, 2, 12, 3), HM_EINVAL);
    expect("energy u16, variant -1 before one frame", e16(w, 2, 5, 250, 1, 12, -1), HM_EINVAL);
    expect("energy u16, one frame before a limit", e16(w, 2, -1, 250, 1, 12, 0), HM_ESHAPE);
    expect("energy u16, 33 frames", e16(w, 2, 5, 250, HM_MAX_FRAMES + 1, 12, 0), HM_ESHAPE);
    expect("energy u16, a limit before no candidates", e16(nullptr, 0, 5, 4096, 2, 12, 0), HM_EINVAL);
    expect("energy u16, no candidates", check_linearity_energy_u16(nullptr, nullptr, nullptr, 0, 0, 4095, 8, 2, 12, 0, nullptr, empty), HM_OK);
    expect("energy u16, no candidates: empty", empty, 1);
    expect("energy u16, no candidates before a row that does not fit", e16(nullptr, 0, 0, 4095, 2, 15, 1), HM_OK);
    expect("energy u16, a row that does not fit before NULL", e16(nullptr, 2, 0, 4095, 2, 15, 1), HM_EUNSUPPORTED);
    expect("energy u16, NULL", check_linearity_energy_u16(nullptr, nullptr, nullptr, 2, 0, 4095, 8, 2, 12, 0, nullptr, empty), HM_EINVAL);
    expect("energy u16, NULL icrf before an odd dn", check_linearity_energy_u16(fake<uint16_t>(0x4001), d, nullptr, 2, 0, 4095, 8, 2, 12, 0, d, empty), HM_EINVAL);
    expect("energy u16, odd dn", e16(fake<uint16_t>(0x4001), 2, 0, 4095, 2, 12, 0), HM_EALIGN);
    expect("energy u16 describe, counts only", check_linearity_energy_u16_counts(2, 0, 0, 8, 2, 12, 0, empty), HM_OK);
    auto de = [&](int pop, int params, int frames) {
        return check_de_generation(1, d, d, d, d, d, b, s, d, d, d, d, b, d, 8, frames, 5, 250, pop, params, 10, 0.5, 1.0, 0.7, 0.01, 0.0);
    };
    expect("de", de(4, 1, 2), HM_OK);
    expect("de, at the limits", de(HM_DE_MAX_POP, HM_DE_MAX_PARAMS, HM_MAX_FRAMES), HM_OK);
    expect("de, population beyond", de(HM_DE_MAX_POP + 1, 1, 2), HM_ESHAPE);
    expect("de, parameters beyond", de(4, HM_DE_MAX_PARAMS + 1, 2), HM_ESHAPE);
    expect("de, NULL status", check_de_generation(1, d, d, d, d, d, b, nullptr, d, d, d, d, b, d, 8, 2, 5, 250, 4, 1, 10, 0.5, 1.0, 0.7, 0.01, 0.0),
           HM_EINVAL);
    expect("de, NaN limit", check_de_generation(1, d, d, d, d, d, b, s, d, d, d, d, b, d, 8, 2, 5, 250, 4, 1, 10, 0.5, 1.0, 0.7, 0.01, kNaN), HM_EINVAL);
    for (int K : {1, 2, HM_DE_MAX_PROBLEMS}) {
        std::vector<const uint8_t*> dn(K, b);
        std::vector<const double*> sd(K, d);
        std::vector<int64_t> seeds(K, 1);
        auto batch = [&](int n_problems, int pop, const double* const* stds, const int64_t* sp) {
            return check_de_generation_batch(n_problems, d, d, d, d, d, b, s, d, d, d, d, dn.data(), stds, sp, d, 8, 2, 5, 250, pop, 1, 10, 0.5, 1.0, 0.7,
                                             0.01, 0.0);
        };
        expect("batch", batch(K, 4, sd.data(), seeds.data()), HM_OK);
        expect("batch, no stds", batch(K, 4, nullptr, seeds.data()), HM_OK);
        expect("batch, no seeds", batch(K, 4, sd.data(), nullptr), HM_EINVAL);
        expect("batch, too many problems", batch(HM_DE_MAX_PROBLEMS + 1, 4, sd.data(), seeds.data()), HM_ESHAPE);
        expect("batch, no problems", batch(0, 4, sd.data(), seeds.data()), HM_EINVAL);
        expect("batch, candidates", batch(K, HM_DE_MAX_POP, sd.data(), seeds.data()), K * HM_DE_MAX_POP > kEnergyMaxCandidates ? HM_EUNSUPPORTED : HM_OK);
        sd[K - 1] = nullptr;
        expect("batch, last std NULL", batch(K, 4, sd.data(), seeds.data()), HM_EINVAL);
        dn[K - 1] = nullptr;
        expect("batch, last stack NULL", batch(K, 4, nullptr, seeds.data()), HM_EINVAL);
    }
}

void pairs() {
    using namespace hm_rules;
    double* d = fake<double>(0x1000);
    for (int n : {1, 2, HM_MAX_FRAMES})
        for (int np : {1, 3, 4 * HM_PAIRS_MAX}) {
            std::vector<const double*> vals(n, d), stds(n, d);
            std::vector<int32_t> pi(np, 0), pj(np, n - 1);
            std::vector<double> mult(np, 1.0);
            auto stat = [&](int frames, int n_pairs, const double* const* sd) {
                return check_pairs(vals.data(), sd, frames, pi.data(), pj.data(), mult.data(), n_pairs, 12, 3, nullptr, nullptr, d, d);
            };
            expect("pairs", stat(n, np, stds.data()), HM_OK);
            expect("pairs, no stds", stat(n, np, nullptr), HM_OK);
            expect("pairs, too many frames", stat(HM_MAX_FRAMES + 1, np, stds.data()), HM_EINVAL);
            expect("pairs, no pairs", stat(n, 0, stds.data()), HM_EINVAL);
            expect("pairs histogram", check_pairs_histogram(vals.data(), stds.data(), n, pi.data(), pj.data(), mult.data(), np, 12, 3, 7, nullptr, nullptr, d,
                                                            HM_PAIRS_HIST_MAX_BINS, d, d), HM_OK);
            expect("pairs histogram, bins beyond", check_pairs_histogram(vals.data(), stds.data(), n, pi.data(), pj.data(), mult.data(), np, 12, 3, 7, nullptr,
                                                                         nullptr, d, HM_PAIRS_HIST_MAX_BINS + 1, d, d), HM_EINVAL);
            pj[np - 1] = n;
            expect("pairs, last index out of range", stat(n, np, stds.data()), HM_EINVAL);
            stds[n - 1] = fake<double>(0x1004);
            expect("pairs, last std misaligned", stat(n, np, stds.data()), HM_EALIGN);
            vals[n - 1] = nullptr;
            expect("pairs, last frame NULL", stat(n, np, stds.data()), HM_EINVAL);
        }
    expect("pairs, NULL arrays", check_pairs(nullptr, nullptr, 2, nullptr, nullptr, nullptr, 1, 12, 3, nullptr, nullptr, d, d), HM_EINVAL);
    expect("pairs, C = 0", check_pairs(nullptr, nullptr, 2, nullptr, nullptr, nullptr, 1, 12, 0, nullptr, nullptr, d, d), HM_EINVAL);
}

void tiff() {
    using namespace hm_rules;
    uint8_t* b = fake<uint8_t>(0x1000);
    int64_t* s = fake<int64_t>(0x2000);
    TiffDecodeGeom dg;
    expect("decode", check_tiff_decode(b, 48, s, s, 2, 5, 1, 2, 4, 4, 3, 1, 0, b, s, b, dg), HM_OK);
    expect("decode: strip bytes", dg.strip_bytes, 24);
    expect("decode, NULL", check_tiff_decode(nullptr, 48, nullptr, nullptr, 2, 5, 1, 2, 4, 4, 3, 1, 0, nullptr, nullptr, nullptr, dg), HM_EINVAL);
    expect("decode, no rows per strip", check_tiff_decode(b, 48, s, s, 2, 5, 1, 0, 4, 4, 3, 1, 0, b, s, b, dg), HM_EINVAL);       // no division by rps = 0
    const int big = std::numeric_limits<int>::max();
    expect("decode, largest ints", check_tiff_decode(b, 48, s, s, 1, 1, 1, big, big, big, 4, 8, 0, b, s, b, dg), HM_ESHAPE);      // no overflow
    expect("decode, a 2^31-byte strip", check_tiff_decode(b, 48, s, s, 2, 1, 1, 2, 4, 1 << 30, 1, 1, 0, b, s, nullptr, dg), HM_OK);
    expect("decode, beyond it", check_tiff_decode(b, 48, s, s, 2, 1, 1, 2, 4, (1 << 30) + 1, 1, 1, 0, b, s, nullptr, dg), HM_ESHAPE);
    TiffEncodeGeom eg;
    const int64_t cap = std::numeric_limits<int64_t>::max();
    expect("encode", check_tiff_encode(b, 0, 1.0, 4, 4, 3, 2, 5, 1, b, cap, s, s, b, eg), HM_OK);
    expect("encode: strips", eg.n_strips, 2);
    expect("encode: pitches", eg.in_pitch + eg.out_pitch, round16(24) + round16(hm_lzw_enc::bound(24)));
    expect("encode, NULL", check_tiff_encode(nullptr, 0, 1.0, 4, 4, 3, 2, 5, 1, nullptr, cap, nullptr, nullptr, nullptr, eg), HM_EINVAL);
    expect("encode, no rows per strip", check_tiff_encode(b, 0, 1.0, 4, 4, 3, 0, 5, 1, b, cap, s, s, b, eg), HM_EINVAL);
    expect("encode, largest ints", check_tiff_encode(b, 1, 1.0, big, big, 4, big, 1, 1, b, cap, s, s, b, eg), HM_ESHAPE);
    expect("encode, a (2^31 - 1)-byte strip", check_tiff_encode(b, 0, 1.0, 4, big, 1, 1, 1, 1, b, cap, s, s, nullptr, eg), HM_OK);
    expect("encode, a 2^31-byte strip", check_tiff_encode(b, 0, 1.0, 4, 1 << 30, 1, 2, 1, 1, b, cap, s, s, nullptr, eg), HM_ESHAPE);
    expect("encode, NaN divisor", check_tiff_encode(b, 2, kNaN, 4, 4, 3, 2, 5, 1, b, cap, s, s, b, eg), HM_EINVAL);
    expect("encode wide", check_tiff_encode_wide(b, HM_TIFF_SRC_U16, 1.0, 0, 4, 4, 3, 2, 5, 2, b, cap, s, s, b, eg), HM_OK);
    expect("encode wide: pitches", eg.in_pitch + eg.out_pitch, round16(48) + round16(hm_lzw_enc::bound(48)));
    expect("encode wide, NULL", check_tiff_encode_wide(nullptr, 0, 1.0, 0, 4, 4, 3, 2, 5, 1, nullptr, cap, nullptr, nullptr, nullptr, eg), HM_EINVAL);
    expect("encode wide, no rows per strip", check_tiff_encode_wide(b, 0, 1.0, 0, 4, 4, 3, 0, 5, 1, b, cap, s, s, b, eg), HM_EINVAL);
    expect("encode wide, largest ints", check_tiff_encode_wide(b, HM_TIFF_SRC_F32, 1.0, 0, big, big, 4, big, 1, 1, b, cap, s, s, b, eg), HM_ESHAPE);
    expect("encode wide, a (2^31 - 2)-byte strip", check_tiff_encode_wide(b, 0, 1.0, 0, 4, (1 << 30) - 1, 1, 1, 1, 1, b, cap, s, s, nullptr, eg), HM_OK);
    expect("encode wide, a 2^31-byte strip", check_tiff_encode_wide(b, 0, 1.0, 0, 4, 1 << 30, 1, 1, 1, 1, b, cap, s, s, nullptr, eg), HM_ESHAPE);
    expect("encode wide, NaN divisor", check_tiff_encode_wide(b, HM_TIFF_SRC_F64_AS_U16, kNaN, 4095, 4, 4, 3, 2, 5, 1, b, cap, s, s, b, eg), HM_EINVAL);
    expect("encode wide, max_dn 65536", check_tiff_encode_wide(b, HM_TIFF_SRC_F64_AS_U16, 1.0, 65536, 4, 4, 3, 2, 5, 1, b, cap, s, s, b, eg), HM_EINVAL);
    expect("encode wide, NaN divisor not read", check_tiff_encode_wide(b, HM_TIFF_SRC_F64_AS_F32, kNaN, -1, 4, 4, 3, 2, 5, 1, b, cap, s, s, b, eg), HM_OK);
    expect("bound(0)", tiff_encode_bound(0), HM_EINVAL);
    expect("bound(2^31)", tiff_encode_bound(int64_t{1} << 31), HM_ESHAPE);
    expect("bound(2^31 - 1)", tiff_encode_bound(kTiffEncodeMaxStripBytes), hm_lzw_enc::bound(kTiffEncodeMaxStripBytes));
    expect("payload, most strips of the largest size", tiff_encode_payload_bytes(big, kTiffEncodeMaxStripBytes, 5) > 0, 1);     // no overflow
    expect("workspace, most strips of the largest size", tiff_encode_workspace_bytes(big, kTiffEncodeMaxStripBytes, 5) > 0, 1);
    expect("decode workspace, at the limit", static_cast<long long>(tiff_decode_workspace_bytes(1, kTiffDecodeMaxStripBytes, 5)), 1ll << 31);
    expect("decode workspace, beyond", static_cast<long long>(tiff_decode_workspace_bytes(1, kTiffDecodeMaxStripBytes + 1, 5)), 0);
}

constexpr int64_t kHuge = int64_t{1} << 62;

void per_frame() {
    using namespace hm_rules;
    double* d = fake<double>(0x1000);
    double* odd = fake<double>(0x1004);
    uint8_t* b = fake<uint8_t>(0x2001);
    uint16_t* w = fake<uint16_t>(0x3000);
    for (Build build : {DEVICE, HOST}) {
        const bool dev = build == DEVICE;
        for (bool f64in : {false, true}) {
            const void* in = f64in ? static_cast<const void*>(d) : b;
            expect("linearize", check_linearize(f64in, in, d, d, d, d, kHuge, 3, 3, build), HM_OK);
            expect("linearize, no table and nothing to do", check_linearize(f64in, in, d, nullptr, d, d, 0, 3, 3, build), dev ? HM_EINVAL : HM_OK);
            expect("linearize, no table", check_linearize(f64in, in, d, nullptr, d, d, 12, 3, 3, build), HM_EINVAL);
            expect("linearize, 5 tables", check_linearize(f64in, in, d, d, d, d, 12, 5, 5, build), dev ? HM_EUNSUPPORTED : HM_OK);
            expect("linearize, 5 channels on one table", check_linearize(f64in, in, d, d, d, d, 12, 5, 1, build), HM_OK);
            expect("linearize, 5 tables and nothing to do", check_linearize(f64in, nullptr, d, d, nullptr, d, 0, 5, 5, build), dev ? HM_EUNSUPPORTED : HM_OK);
            expect("linearize, misaligned std", check_linearize(f64in, in, odd, d, d, nullptr, 12, 3, 3, build), dev ? HM_EALIGN : HM_OK);
            expect("linearize, misaligned input", check_linearize(f64in, f64in ? static_cast<const void*>(odd) : b, d, d, d, d, 12, 3, 3, build),
                   dev && f64in ? HM_EALIGN : HM_OK);
        }
    }
    expect("linearize u16", check_linearize_u16(w, d, d, d, d, w, kHuge, 3, 3, 16), HM_OK);
    expect("linearize u16, optional NULLs", check_linearize_u16(w, nullptr, d, d, nullptr, nullptr, 12, 3, 1, 9), HM_OK);
    expect("linearize u16, 8 bits", check_linearize_u16(w, d, d, d, d, w, 12, 3, 3, 8), HM_EINVAL);
    expect("linearize u16, odd dn", check_linearize_u16(fake<uint16_t>(0x3001), d, d, d, d, w, 12, 3, 3, 12), HM_EALIGN);
    expect("linearize u16, odd dn and nothing to do", check_linearize_u16(fake<uint16_t>(0x3001), d, d, d, d, w, 0, 3, 3, 12), HM_OK);
    std::vector<double> w8(256), w8b(256), w16(65536);
    expect("weight table", gaussian_weight_lut(8, w8.data(), nullptr), HM_OK);
    expect("weight table, 16 bits", gaussian_weight_lut(16, w16.data(), w16.data()), HM_OK);
    expect("weight table, 7 bits", gaussian_weight_lut(7, w8.data(), w8b.data()), HM_EINVAL);
    expect("weight table, NULL", gaussian_weight_lut(8, nullptr, nullptr), HM_EINVAL);
}

void operators() {
    using namespace hm_rules;
    int64_t n;
    double* d = fake<double>(0x1000);
    double* odd = fake<double>(0x1004);
    const int big = std::numeric_limits<int>::max();
    for (Build build : {DEVICE, HOST}) {
        const bool dev = build == DEVICE;
        for (int ndim : {1, HM_MAX_DIMS}) {
            std::vector<int64_t> shape(ndim, 3), st(ndim, 1);
            auto bin = [&](const double* x1, const double* out_std) {
                return check_binary_op(HM_OP_POW, x1, d, d, nullptr, d, out_std, ndim, shape.data(), st.data(), st.data(), build, n);
            };
            expect("binary", bin(d, d), HM_OK);
            expect("binary: n", n, ndim == 1 ? 3 : 729);
            expect("binary, std in, none out", bin(d, nullptr), HM_EINVAL);
            expect("binary, misaligned", bin(odd, d), dev ? HM_EALIGN : HM_OK);
            expect("difference", check_compute_difference_bcast(d, d, d, nullptr, d, d, d, d, ndim, shape.data(), st.data(), st.data(), n), HM_OK);
            expect("interpolate", check_interpolate_bcast(d, nullptr, d, d, d, d, ndim, shape.data(), st.data(), st.data(), n), HM_OK);
            shape[ndim - 1] = kHuge;                                                     // 2^62, or 3^5 x 2^62: beyond int64
            expect("binary, 2^62 in the last extent", bin(d, d), ndim == 1 ? HM_OK : HM_EINVAL);
            expect("difference, 2^62 in the last extent",
                   check_compute_difference_bcast(d, d, d, nullptr, d, d, d, d, ndim, shape.data(), st.data(), st.data(), n), ndim == 1 ? HM_OK : HM_EINVAL);
            shape[0] = 0;                                                                // no element, whatever the other extents
            expect("binary, an extent of 0", bin(d, d), HM_OK);
                    expect("interpolate, an extent of 0, NULL operands",
                   check_interpolate_bcast(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ndim, shape.data(), st.data(), st.data(), n), HM_OK);
            st[ndim - 1] = -1;
            expect("binary, misaligned before a negative stride", bin(odd, d), dev ? HM_EALIGN : HM_EINVAL);
            expect("binary, negative last stride", bin(d, d), HM_EINVAL);
            expect("binary, one dimension too many", check_binary_op(HM_OP_ADD, d, d, d, d, d, d, ndim + HM_MAX_DIMS, shape.data(), st.data(), st.data(), build, n),
                   HM_EINVAL);
        }
        expect("binary, NULL arrays", check_binary_op(HM_OP_ADD, d, d, d, d, d, d, 2, nullptr, nullptr, nullptr, build, n), HM_EINVAL);
        expect("unary", check_unary_op(HM_UOP_LOG_10, d, d, d, d, kHuge, build), HM_OK);
        expect("unary, unknown", check_unary_op(HM_UOP_LOG_10 + 1, d, d, d, d, 0, build), HM_EINVAL);
        expect("unary, NULL and nothing to do", check_unary_op(HM_UOP_NEG, nullptr, nullptr, nullptr, nullptr, 0, build), HM_OK);
        expect("pow, misaligned", check_unary_op(HM_UOP_NEG, d, nullptr, odd, nullptr, 12, build), dev ? HM_EALIGN : HM_OK);
        expect("pow, std in, none out", check_unary_op(HM_UOP_NEG, d, d, d, nullptr, 12, build), HM_EINVAL);
        for (int count : {1, HM_TAKE_MAX, HM_TAKE_MAX + 1}) {
            std::vector<int64_t> indices(count, -3), idx(count);
            auto take = [&](int n_indices, int64_t outer) {
                return check_take_axis(d, nullptr, d, nullptr, outer, 3, kHuge, indices.data(), n_indices, build, [&] { return idx.data(); });
            };
            const int ok = dev && count > HM_TAKE_MAX ? HM_EUNSUPPORTED : HM_OK;
            expect("take", take(count, 2), ok);
            if (ok == HM_OK) expect("take: normalised", idx[count - 1] == 0, 1);
            expect("take, no planes", take(count, 0), ok);
            indices[count - 1] = 3;
            expect("take, last index out of range", take(count, 2), ok == HM_OK ? HM_ESHAPE : ok);
            indices[count - 1] = std::numeric_limits<int64_t>::min();
            expect("take, last index the smallest int64", take(count, 2), ok == HM_OK ? HM_ESHAPE : ok);
        }
        bool asked = false;                                                          // a refused call asks for no room
        auto no_room = [&]() -> int64_t* { asked = true; return nullptr; };
        expect("take, no indices", check_take_axis(d, d, d, d, 2, 3, 2, nullptr, 3, build, no_room), HM_EINVAL);
        expect("take, the most indices an int counts and no x", check_take_axis(nullptr, d, d, d, 2, 3, 2, fake<int64_t>(0x2000), big, build, no_room), HM_EINVAL);
        expect("take, the most indices an int counts", check_take_axis(d, d, d, nullptr, 2, 3, 2, fake<int64_t>(0x2000), big, build, no_room),
               dev ? HM_EUNSUPPORTED : HM_EINVAL);
        expect("take, refused: no room asked for", asked, 0);
        expect("thresholds", check_apply_thresholds(d, d, d, d, kHuge, HM_THRESHOLD_MAX_CHANNELS, build), HM_OK);
        expect("thresholds, 33 channels", check_apply_thresholds(d, d, d, d, 12, HM_THRESHOLD_MAX_CHANNELS + 1, build), HM_EUNSUPPORTED);
        expect("thresholds, most channels an int counts", check_apply_thresholds(nullptr, d, d, d, 0, big, build), HM_EUNSUPPORTED);
        expect("thresholds, misaligned std", check_apply_thresholds(d, odd, d, d, 12, 3, build), dev ? HM_EALIGN : HM_OK);
    }
    const int64_t one = 1;                                                               // the 1-D entries: shape = {n}, strides = {1}
    auto diff1 = [&](const double* x, const double* s, const double* out_rel_std, int64_t count) {
        return check_compute_difference_bcast(x, s, x, s, x, s, x, out_rel_std, 1, &count, &one, &one, n);
    };
    expect("difference, 2^62 elements", diff1(d, nullptr, nullptr, kHuge), HM_OK);
    expect("difference, negative count", diff1(d, nullptr, nullptr, -1), HM_EINVAL);
    expect("difference, NULL and nothing to do", diff1(nullptr, nullptr, nullptr, 0), HM_OK);
    expect("difference, one std output", diff1(d, d, nullptr, 12), HM_EINVAL);
    int64_t count = kHuge;
    expect("interpolate, 2^62 elements", check_interpolate_bcast(d, d, d, nullptr, d, d, 1, &count, &one, &one, n), HM_OK);
    expect("interpolate, std out, none in", check_interpolate_bcast(d, nullptr, d, nullptr, d, d, 1, &count, &one, &one, n), HM_EINVAL);
}

void statistics() {
    using namespace hm_rules;
    expect("dense elements", dense_elems({2, 3, 4}), 24);
    expect("dense elements, an extent of 0", dense_elems({2, 0, 4}), -1);
    expect("dense elements, 2^48", dense_elems({int64_t{1} << 16, int64_t{1} << 16, int64_t{1} << 16}), int64_t{1} << 48);
    expect("dense elements, beyond", dense_elems({int64_t{1} << 16, (int64_t{1} << 16) + 1, int64_t{1} << 16}), -1);
    expect("dense elements, five extents of 2^62", dense_elems({kHuge, kHuge, kHuge, kHuge, kHuge}), -1);
}

}  // namespace

int main() {
    producers();
    calibration();
    pairs();
    tiff();
    per_frame();
    operators();
    statistics();
    std::printf(failures ? "%d FAILED\n" : "entry rules: all checks passed\n", failures);
    return failures ? 1 : 0;
}
