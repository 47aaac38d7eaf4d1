// merge_rules_check.cpp - the host build's merge _describe entries (camera_linearity_amd/csrc/hm_merge_rules.h through
// csrc_host/hm_host.cpp) under AddressSanitizer / UBSan: the NULL, short-struct_size and n_frames = 33 cases, in which the rules must
// answer without reading past what the caller gave them. A development step for whoever changes that header: a stand-alone program, not
// part of the library, the package or the test suite, and it needs no GPU.
//
//   g++ -std=c++17 -O1 -g -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/merge_rules_check.cpp camera_linearity_amd/csrc_host/hm_host.cpp -o /tmp/merge_rules_check && /tmp/merge_rules_check
#include <cstdio>
#include <cstring>
#include <vector>
#include "hdrmerge.h"

namespace {

int failures = 0;
void expect(const char* what, int got, int want) {
    if (got != want) { std::printf("FAIL %s: %d, expected %d\n", what, got, want); ++failures; }
}

}  // namespace

int main() {
    char buf[256];
    // every array has exactly n entries and the struct is a heap block of exactly struct_size bytes: a read behind either stops the program
    for (int n : {7, 33}) {
        for (uint32_t size : {static_cast<uint32_t>(sizeof(hm_merge_args)), 264u, 100u}) {
            std::vector<const uint8_t*> frames(n, reinterpret_cast<const uint8_t*>(0x100000));
            std::vector<const float*> stds_f32(n, reinterpret_cast<const float*>(0x200000));
            std::vector<const double*> stds(n, reinterpret_cast<const double*>(0x300000));
            std::vector<double> exposures(n, 1e-3);
            hm_merge_args a{};
            a.struct_size = size;
            a.n_frames = n; a.channels = 3;
            a.height = a.rows = a.buf_rows = a.width = 64;
            a.frames_u8 = frames.data(); a.exposures = exposures.data();
            a.icrf = reinterpret_cast<const double*>(0x400000); a.icrf_diff = a.icrf; a.w_lut = a.icrf; a.dw_lut = a.icrf;
            a.out_val = reinterpret_cast<double*>(0x500000); a.out_std = a.out_val;
            std::vector<char> block(size);
            std::memcpy(block.data(), &a, size);
            auto* g = reinterpret_cast<hm_merge_args*>(block.data());
            const int short_rc = size == 100u ? HM_EINVAL : HM_OK;
            // hm_merge (float64 std frames) and hm_merge_std_table take any number of frames on the host; float32 stds stop at HM_MAX_FRAMES
            expect("std_table", hm_merge_std_table_describe(g, a.icrf, buf, sizeof buf), short_rc);
            expect("std_f32", hm_merge_std_f32_describe(g, stds_f32.data(), buf, sizeof buf), size == 100u ? HM_EINVAL : n == 33 ? HM_EUNSUPPORTED : HM_OK);
            expect("std_table, NULL table", hm_merge_std_table_describe(g, nullptr, buf, sizeof buf), HM_EINVAL);
            expect("std_f32, NULL stds", hm_merge_std_f32_describe(g, nullptr, buf, sizeof buf), HM_EINVAL);
            {   // hm_merge_u16: the frames travel beside the struct (frames_u8 must be NULL); the chunked path does not exist for it
                std::vector<const uint16_t*> frames_u16(n, reinterpret_cast<const uint16_t*>(0x600000));
                std::vector<char> block16(block);
                auto* g16 = reinterpret_cast<hm_merge_args*>(block16.data());
                g16->frames_u8 = nullptr;
                if (size != 100u) g16->out_std = nullptr;        // (value-only first; the 100-byte block ends before the field)
                const int rc16 = size == 100u ? HM_EINVAL : n == 33 ? HM_EUNSUPPORTED : HM_OK;
                expect("u16", hm_merge_u16_describe(g16, frames_u16.data(), 12, buf, sizeof buf), rc16);
                expect("u16, 16 bits", hm_merge_u16_describe(g16, frames_u16.data(), 16, buf, sizeof buf), rc16);
                expect("u16, 8 bits", hm_merge_u16_describe(g16, frames_u16.data(), 8, buf, sizeof buf), HM_EINVAL);
                expect("u16, NULL frames", hm_merge_u16_describe(g16, nullptr, 12, buf, sizeof buf), HM_EINVAL);
                expect("u16, frames_u8 set", hm_merge_u16_describe(g, frames_u16.data(), 12, buf, sizeof buf), HM_EINVAL);
                g16->stds = stds.data();
                if (size != 100u) g16->out_std = a.out_std;
                expect("u16 with stds", hm_merge_u16_describe(g16, frames_u16.data(), 10, buf, sizeof buf), rc16);
                if (size != 100u) hm_merge_u16_algorithmic_bytes(g16);
                // hm_merge_u16_std_table: the table beside the struct, args->stds NULL, the maps optional
                const double* table = reinterpret_cast<const double*>(0x700000);
                std::vector<const uint16_t*> darks_u16(n, nullptr);
                expect("u16 table, stds set", hm_merge_u16_std_table_describe(g16, frames_u16.data(), nullptr, table, 12, buf, sizeof buf), HM_EINVAL);
                g16->stds = nullptr;
                expect("u16 table", hm_merge_u16_std_table_describe(g16, frames_u16.data(), nullptr, table, 12, buf, sizeof buf), rc16);
                expect("u16 table, NULL table", hm_merge_u16_std_table_describe(g16, frames_u16.data(), nullptr, nullptr, 12, buf, sizeof buf), HM_EINVAL);
                expect("u16 table, NULL frames", hm_merge_u16_std_table_describe(g16, nullptr, nullptr, table, 12, buf, sizeof buf), HM_EINVAL);
                expect("u16 table, maps without thresholds", hm_merge_u16_std_table_describe(g16, frames_u16.data(), darks_u16.data(), table, 12, buf, sizeof buf),
                       HM_EINVAL);
                if (size != 100u) { hm_merge_u16_std_table_algorithmic_bytes(g16, nullptr); hm_merge_u16_std_table_algorithmic_bytes(g16, darks_u16.data()); }
            }
            g->stds = stds.data();
            expect("merge", hm_merge_describe(g, buf, sizeof buf), short_rc);
            expect("merge, NULL buf", hm_merge_describe(g, nullptr, 0), HM_EINVAL);
            if (size != 100u) {                                  // (the byte count takes the struct on trust: it has no status to refuse one with)
                hm_merge_std_table_algorithmic_bytes(g); hm_merge_std_f32_algorithmic_bytes(g); hm_merge_algorithmic_bytes(g);
            }
        }
    }
    expect("merge, NULL args", hm_merge_describe(nullptr, buf, sizeof buf), HM_EINVAL);
    expect("std_table, NULL args", hm_merge_std_table_describe(nullptr, nullptr, buf, sizeof buf), HM_EINVAL);
    expect("std_f32, NULL args", hm_merge_std_f32_describe(nullptr, nullptr, buf, sizeof buf), HM_EINVAL);
    expect("u16, NULL args", hm_merge_u16_describe(nullptr, nullptr, 12, buf, sizeof buf), HM_EINVAL);
    expect("u16 table, NULL args", hm_merge_u16_std_table_describe(nullptr, nullptr, nullptr, nullptr, 12, buf, sizeof buf), HM_EINVAL);
    if (hm_merge_u16_algorithmic_bytes(nullptr) || hm_merge_u16_std_table_algorithmic_bytes(nullptr, nullptr)) ++failures;
    if (hm_merge_algorithmic_bytes(nullptr) || hm_merge_std_table_algorithmic_bytes(nullptr) || hm_merge_std_f32_algorithmic_bytes(nullptr)) ++failures;
    std::printf(failures ? "merge_rules_check: %d FAILED\n" : "merge_rules_check: ok\n", failures);
    return failures != 0;
}
