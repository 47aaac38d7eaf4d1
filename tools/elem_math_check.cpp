// elem_math_check.cpp - the element formulas that both builds evaluate (camera_linearity_amd/csrc/hm_merge_math.h, hm_ops_math.h,
// hm_stats_math.h, hm_producer_math.h on hm_math_common.h), checked on their own under AddressSanitizer / UBSan: the index linearize
// forms and the uint8 rounding at their wrap and guard points (an unguarded cast of NaN or 1e30 stops the program), the 'reflect' fold
// against a brute-force table, floordiv2, the histogram index at every edge and its neighbours, the uniform draws, and that every
// operator and difference function called without std leaves its std outputs alone and returns the plain expression's value.
// A development step for whoever changes those headers: a stand-alone program, not part of the library, the package or the test suite,
// and it needs no GPU.
//
// Build and run (one command line):
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Icamera_linearity_amd/csrc
//       tools/elem_math_check.cpp -o /tmp/elem_math_check && /tmp/elem_math_check
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "hm_merge_math.h"
#include "hm_ops_math.h"
#include "hm_producer_math.h"
#include "hm_stats_math.h"

namespace {

using namespace hm;

int failures = 0;
void expect(const char* what, long long got, long long want) {
    if (got != want) { std::printf("FAIL %s: %lld, expected %lld\n", what, got, want); ++failures; }
}
// the same float64: equal, or both NaN
void expect_f(const char* what, double got, double want) {
    if (!(got == want || (got != got && want != want))) { std::printf("FAIL %s: %.17g, expected %.17g\n", what, got, want); ++failures; }
}
const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kInf = std::numeric_limits<double>::infinity();

void indices() {
    for (int k = 0; k < 256; ++k) expect("lut_index(k / 255)", lut_index(k / 255.0), k);
    expect("lut_index(-1 / 255)", lut_index(-1.0 / 255.0), 255);                 // wraps modulo 256, negatives included
    expect("lut_index(256 / 255)", lut_index(256.0 / 255.0), 0);
    expect("lut_index(1000 / 255)", lut_index(1000.0 / 255.0), 1000 & 255);
    expect("lut_index(-1000 / 255)", lut_index(-1000.0 / 255.0), 24);
    expect("lut_index(1e30)", lut_index(1e30), 0);                               // beyond +-9.2e18 and NaN: 0, no cast
    expect("lut_index(-1e30)", lut_index(-1e30), 0);
    expect("lut_index(+inf)", lut_index(kInf), 0);
    expect("lut_index(-inf)", lut_index(-kInf), 0);
    expect("lut_index(NaN)", lut_index(kNaN), 0);

    const struct { double x; int want; } r8[] = {{0.5, 0}, {1.5, 2}, {2.5, 2}, {254.5, 254}, {255.5, 0}, {-0.5, 0}, {256.0, 0}, {-1.0, 255},
                                                 {1e30, 0}, {-1e30, 0}, {kNaN, 0}, {kInf, 0}, {-kInf, 0}, {127.0, 127}, {255.0, 255}};
    for (const auto& c : r8) expect("round_to_u8", round_to_u8(c.x), c.want);    // half to even, low byte, 0 beyond +-9.2e18 and for NaN

    for (int n = 1; n <= 5; ++n)                                                 // d c b a | a b c d | d c b a: period 2n
        for (int i = -3 * n; i <= 3 * n; ++i) {
            const int m = ((i % (2 * n)) + 2 * n) % (2 * n);
            expect("reflect_index", reflect_index(i, n), m < n ? m : 2 * n - 1 - m);
        }
    for (int x = -5; x <= 5; ++x) expect("floordiv2", floordiv2(x), static_cast<long long>(floor(x / 2.0)));
}

void histogram() {
    const double ranges[2][2] = {{0.0, 1.0}, {-3.0, 5.0}};
    for (const auto& rg : ranges)
        for (int bins : {1, 2, 7}) {
            const double lo = rg[0], hi = rg[1], norm = static_cast<double>(bins) / (hi - lo);
            std::vector<double> edges(bins + 1);                                  // a heap block of exactly bins + 1 edges
            for (int j = 0; j <= bins; ++j) edges[j] = lo + (hi - lo) * j / bins;
            for (int j = 0; j <= bins; ++j)
                for (const double x : {nextafter(edges[j], -kInf), edges[j], nextafter(edges[j], kInf)}) {
                    if (!hist_in_range(x, lo, hi)) continue;
                    int want = 0;                                                 // left-closed bins, the last one closed on the right
                    for (int b = 1; b < bins; ++b) if (x >= edges[b]) want = b;
                    const int got = hist_bin(x, lo, norm, edges.data(), bins), got_b = hist_bin_bounded(x, lo, norm, edges.data(), bins);
                    expect("hist_bin", got, want);
                    expect("hist_bin_bounded", got_b, want);
                    expect("hist_bin inside 0..bins-1", got >= 0 && got < bins, 1);
                }
            expect("hist_in_range below", hist_in_range(nextafter(lo, -kInf), lo, hi), 0);
            expect("hist_in_range above", hist_in_range(nextafter(hi, kInf), lo, hi), 0);
        }
    expect("hist_in_range NaN", hist_in_range(kNaN, 0.0, 1.0), 0);
    expect("hist_finite", hist_finite(1.0) && hist_finite(-1e308) && !hist_finite(kInf) && !hist_finite(-kInf) && !hist_finite(kNaN), 1);
    double w = -7.0;
    expect("hist_weight(0)", hist_weight(0.0, w), 0);
    expect_f("hist_weight(0) leaves w", w, -7.0);
    expect("hist_weight(0.25)", hist_weight(0.25, w), 1);
    expect_f("hist_weight(0.25) w", w, 4.0);
    const double val[4] = {1.5, kInf, kNaN, 2.0}, sd[4] = {0.5, 1.0, 1.0, 0.0};
    double x;
    expect("kde_load", kde_load(val, sd, 0, x, w) && x == 1.5 && w == 2.0, 1);
    expect("kde_load inf", kde_load(val, sd, 1, x, w), 0);
    expect("kde_load NaN", kde_load(val, sd, 2, x, w), 0);
    expect("kde_load std 0", kde_load(val, sd, 3, x, w), 0);
    expect("kde_load no std", kde_load(val, nullptr, 3, x, w) && w == 1.0, 1);
}

void draws() {
    const uint64_t key = mix64(0x1234u ^ mix64(7u));
    for (int d = 0; d < 1000; ++d) {
        const int i = d % 37, k = d / 37;
        const double u = de_uniform(key, i, k);
        expect("de_uniform in [0, 1)", u >= 0.0 && u < 1.0, 1);
        expect_f("de_uniform repeats", de_uniform(key, i, k), u);
    }
    expect("de_uniform differs between members", de_uniform(key, 0, 0) != de_uniform(key, 1, 0), 1);
}

// with_std = false: the std outputs keep the caller's value, the result is the plain expression
void without_std() {
    const double kept = -7.0;
    const double xs[] = {1.7, -0.3, 0.0, -0.0, 2.0, 1e30, kInf, -kInf, kNaN};
    for (const double x1 : xs)
        for (const double x2 : {0.5, -2.0, 3.0, 0.0, kNaN}) {
            double r, rs = kept;
            binary_eval<HM_OP_ADD>(x1, 9.0, x2, 9.0, false, r, rs); expect_f("add", r, x1 + x2);
            binary_eval<HM_OP_SUB>(x1, 9.0, x2, 9.0, false, r, rs); expect_f("sub", r, x1 - x2);
            binary_eval<HM_OP_MUL>(x1, 9.0, x2, 9.0, false, r, rs); expect_f("mul", r, x1 * x2);
            binary_eval<HM_OP_DIV>(x1, 9.0, x2, 9.0, false, r, rs); expect_f("div", r, x1 / x2);
            binary_eval<HM_OP_POW>(x1, 9.0, x2, 9.0, false, r, rs); expect_f("pow", r, pow(x1, x2));
            expect_f("binary_eval leaves rs", rs, kept);
            double a, rel, as = kept, rls = kept;
            diff_terms(x1, x2, 9.0, 9.0, 1.9, false, a, rel, as, rls);
            expect_f("diff_terms abs", a, x1 - 1.9 * x2);
            expect_f("diff_terms rel", rel, (x1 - 1.9 * x2) / (1.9 * x2));
            expect_f("diff_terms leaves abs std", as, kept);
            expect_f("diff_terms leaves rel std", rls, kept);
        }
    for (const double x : xs) {
        double r, rs = kept;
        const auto no_std = []() -> double { std::printf("FAIL unary_eval read the std without with_std\n"); std::exit(1); };
        unary_eval(HM_UOP_NEG, x, false, no_std, r, rs); expect_f("neg", r, -x);
        unary_eval(HM_UOP_LOG_E, x, false, no_std, r, rs); expect_f("log_e", r, log(x));
        unary_eval(HM_UOP_LOG_10, x, false, no_std, r, rs); expect_f("log_10", r, log10(x));
        pow_scalar_eval<POW_SQUARE>(x, 9.0, 2.0, 0, false, r, rs); expect_f("pow 2", r, x * x);
        pow_scalar_eval<POW_ONE>(x, 9.0, 1.0, 0, false, r, rs); expect_f("pow 1", r, x);
        pow_scalar_eval<POW_INT>(x, 9.0, 3.0, 3, false, r, rs); expect_f("pow 3", r, (x * x) * x);
        pow_scalar_eval<POW_INT>(x, 9.0, -2.0, -2, false, r, rs); expect_f("pow -2", r, 1.0 / (x * x));
        pow_scalar_eval<POW_GENERAL>(x, 9.0, 1.7, 0, false, r, rs); expect_f("pow 1.7", r, pow(x, 1.7));
        pow_scalar_eval<POW_SQRT>(x, 9.0, 0.5, 0, false, r, rs);
        expect_f("pow 0.5", r, x == -kInf ? kInf : sqrt(x == 0.0 ? 0.0 : x));      // NumPy's pow: -inf -> +inf, -0.0 -> +0.0
        expect_f("unary_eval / pow_scalar_eval leave rs", rs, kept);
        double val = x, sd = kept;
        flat_field_math(0.8, 1.0, 9.0, 0.6, 9.0, false, val, sd);
        expect_f("flat_field_math value", val, (x / 0.8) * 0.6);
        expect_f("flat_field_math leaves sd", sd, kept);
        double ov, os = kept;
        flat_field_exact(x, 9.0, 0.8, 9.0, 0.6, 9.0, false, ov, os);
        expect_f("flat_field_exact value", ov, (x / 0.8) * 0.6);
        expect_f("flat_field_exact leaves os", os, kept);
    }
    // with std: the formulas against their plain expressions at one point
    double r, rs;
    unary_eval(HM_UOP_LOG_10, 3.0, true, [] { return 0.25; }, r, rs);
    expect_f("log_10 std", rs, 0.25 / (3.0 * 0x1.26bb1bbb55515p+1));
    const double w = 0.7, dw = -1.3, g = 0.4, dg = 0.02, S = 2.5, it = 50.0;
    expect_f("merge_var_term", merge_var_term(w, dw, g, dg, 1.0 / S, 1.0 / (S * S), it),
             (((dw * g + w * dg) * (1.0 / S) - ((dw * w) * g) * (1.0 / (S * S))) * dg) * it);
    expect_f("gauss_dweight", gauss_dweight(0.2, gauss_weight(0.2)), (-60.0 * 0.2) * exp(-30.0 * (0.2 * 0.2)));
    const InterpCoef k = interp_coef(0.01, 0.08, 0.03);
    expect_f("interp_value", interp_value(k, 2.0, 5.0), (2.0 * (0.08 - 0.03) + 5.0 * (0.03 - 0.01)) / (0.08 - 0.01));
}

// clean_edges_row on a heap row of exactly 256 bins: no access outside it for any centre
void clean_edges() {
    for (int center = 0; center < 256; ++center) {
        std::vector<int64_t> row(256);
        for (int m = 0; m < 256; ++m) row[m] = (m * 37 + center * 11) % 5 == 0 ? 0 : 100 - (m > center ? m - center : center - m) % 100;
        clean_edges_row([&](int m) -> int64_t& { return row.at(static_cast<size_t>(m)); }, center);
    }
}

}  // namespace

int main() {
    indices();
    histogram();
    draws();
    without_std();
    clean_edges();
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("elem_math_check: all passed\n");
    return 0;
}
