// hm_ops_math.h - the element formulas of the Measurand operators and of the pointwise linearity steps, one text for the device units
// (hm_ops.hip, hm_pointwise.hip, hm_stats_hist.hip) and ../csrc_host/hm_host.cpp: first-order uncertainty propagation in the formulas
// and operation order of modules/measurand.py:106-279 (add / sub / mul / div / pow, neg / log_e / log_10, pow with a scalar exponent),
// :634-653 (ExposurePair difference terms) and :665-679 (interpolate). An std output is written only where the formula has one: a
// function called with with_std = false leaves its std outputs as the caller set them.
//
// DEVICE / HOST - where the two builds perform different operations, on purpose; no output bit of either build moves here:
//   pow_scalar_eval     POW_INT (x ** p for an integer |p| <= 8 by repeated multiplication) is chosen by the DEVICE build only; the host
//                       build sends every exponent but 2, 0.5 and 1 through POW_GENERAL, pow() twice.
#pragma once
#include "hdrmerge.h"
#include "hm_math_common.h"

namespace hm {

template <int OP>
HM_MATH_FN void binary_eval(double x1, double s1, double x2, double s2, bool with_std, double& r, double& rs) {
    if (OP == HM_OP_ADD) {                                  // measurand.py:114,126
        r = x1 + x2;
        if (with_std) rs = sqrt((s1 * s1) + (s2 * s2));
    } else if (OP == HM_OP_SUB) {                           // :138,149
        r = x1 - x2;
        if (with_std) rs = sqrt((s1 * s1) + (s2 * s2));
    } else if (OP == HM_OP_MUL) {                           // :198,209
        r = x1 * x2;
        if (with_std) { const double a = x1 * s2, b = x2 * s1; rs = sqrt(a * a + b * b); }
    } else if (OP == HM_OP_DIV) {                           // :173,184-186
        r = x1 / x2;
        if (with_std) { const double u1 = s1 / x2, u2 = (x1 * s2) / (x2 * x2); rs = sqrt(u1 * u1 + u2 * u2); }
    } else {                                                // pow :225,236-239
        r = pow(x1, x2);
        if (with_std) {
            const double u1 = x2 * pow(x1, x2 - 1.0);
            const double u2 = log(x1) * r;
            const double a = u1 * s1, b = u2 * s2;
            rs = sqrt(a * a + b * b);
        }
    }
}

// neg / log_e / log_10 of a loaded value. s() reads the operand's std: called once, and only with with_std, where the formula uses it.
template <typename LoadStd> HM_MATH_FN void unary_eval(int op, double v, bool with_std, LoadStd s, double& r, double& rs) {
    const double ln10 = 0x1.26bb1bbb55515p+1;              // fl(log 5) + fl(log 2), the constant measurand.py:277 forms
    if (op == HM_UOP_NEG) { r = -v; if (with_std) rs = s(); }                               // :154-157
    else if (op == HM_UOP_LOG_E) { r = log(v); if (with_std) rs = s() / r; }                // :251,258 (as written)
    else { r = log10(v); if (with_std) rs = s() / (v * ln10); }                             // :270,277
}

// x ** p for a plain scalar exponent p (Measurand.__pow__, modules/measurand.py:217-241) with the exponent's kind known to the caller:
//   value:  p == 2 -> x*x,  p == 0.5 -> sqrt(x),  p == 1 -> x,  small integer p -> repeated multiplication, else pow(x, p)
//   std  :  |dx**p/dx| * s = (p * x**(p-1)) * s, with x**(p-1) = x, 1/sqrt(x)... formed from the value; the exponent's term
//           (ln x * x**p * 0)**2 of :236-239 is +0 whenever ln x * x**p is finite and is evaluated as written otherwise
//           (x <= 0 or non-finite: NumPy gives NaN / inf there and so does this).
enum { POW_SQUARE = 0, POW_SQRT = 1, POW_ONE = 2, POW_INT = 3, POW_GENERAL = 4 };

template <int KIND>
HM_MATH_FN void pow_scalar_eval(double x, double s, double p, int ip, bool with_std, double& r, double& rs) {
    double d;                                               // x ** (p - 1)
    if (KIND == POW_SQUARE) { r = x * x; d = x; }
    else if (KIND == POW_SQRT) {                            // sqrt: the correctly rounded x ** 0.5. NumPy's pow() differs from it at two arguments only:
        const double ax = (x == 0.0 || x == -__builtin_huge_val()) ? fabs(x) : x;       // -inf -> +inf (d = +0) and -0.0 -> +0.0 (d = +inf)
        r = sqrt(ax); d = 1.0 / r;
    }
    else if (KIND == POW_ONE) { r = x; d = 1.0; }
    else if (KIND == POW_INT) {                             // |ip| <= 8: x**(|ip|-1) by multiplication, one more for the value
        const int n = ip < 0 ? -ip : ip;
        double acc = 1.0;
        for (int k = 1; k < n; ++k) acc *= x;
        if (ip > 0) { d = acc; r = acc * x; }
        else { r = 1.0 / (acc * x); d = r / x; }
    } else { r = pow(x, p); d = pow(x, p - 1.0); }
    if (with_std) {
        const double a = (p * d) * s;                        // measurand.py:236
        double b = 0.0;                                      // (log(x1) * x1**x2) * 0, :237-238
        const double lr = r;
        if (!(x > 0.0) || !(fabs(x) < __builtin_huge_val()) || !(fabs(lr) < __builtin_huge_val())) b = (log(x) * r) * 0.0;
        rs = sqrt(a * a + b * b);
    }
}

// ExposurePair difference terms of one element (measurand.py:634-653): the absolute difference a = x - mult y, the relative one
// r = a / (mult y), and their stds
HM_MATH_FN double diff_abs(double xv, double yv, double mult) { return xv - mult * yv; }            // :634-635
HM_MATH_FN double diff_rel(double a, double yv, double mult) { return a / (mult * yv); }            // :636
HM_MATH_FN double diff_abs_std(double xs, double ys, double mult) {
    const double m1 = mult * ys;
    return sqrt(xs * xs + m1 * m1);                         // :652
}
HM_MATH_FN double diff_rel_std(double xv, double yv, double xs, double ys, double mult) {
    const double u1 = xs / (mult * yv);
    const double u2 = (ys * xv) / (mult * (yv * yv));
    return sqrt(u1 * u1 + u2 * u2);                         // :653
}
HM_MATH_FN void diff_terms(double xv, double yv, double xs, double ys, double mult, bool with_std, double& a, double& r, double& as, double& rs) {
    a = diff_abs(xv, yv, mult);
    r = diff_rel(a, yv, mult);
    if (with_std) { as = diff_abs_std(xs, ys, mult); rs = diff_rel_std(xv, yv, xs, ys, mult); }
}

// interpolate between two measurands at y0 < y < y1 (measurand.py:657-681): the call's coefficients, then value and std of one element
struct InterpCoef { double a, b, d, ca, cb; };
HM_MATH_FN InterpCoef interp_coef(double y0, double y1, double y) {
    const double a = y1 - y, b = y - y0, d = y1 - y0;
    return InterpCoef{a, b, d, (a / d) * (a / d), (b / d) * (b / d)};
}
HM_MATH_FN double interp_value(const InterpCoef& k, double x0, double x1) { return (x0 * k.a + x1 * k.b) / k.d; }              // :665
HM_MATH_FN double interp_std(const InterpCoef& k, double s0, double s1) { return sqrt(s0 * k.ca + s1 * k.cb); }                // :679 as written

}  // namespace hm
