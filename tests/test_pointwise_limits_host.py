"""The operator, selection and per-frame kernels at the limits of their ABI: hm_binary_op / hm_unary_op / hm_pow_scalar / hm_take_axis
(csrc/hm_ops.hip), hm_apply_thresholds / hm_compute_difference / hm_interpolate and the two _bcast entries (csrc/hm_pointwise.hip),
hm_u8_to_unit_f64 / hm_gaussian_weight_f64 / _u8 / hm_linearize_u8 / _f64 / _u16 (csrc/hm_linearize.hip), on the HOST build
(csrc_host/hm_host.cpp). The checks are functions of a device name: tests/test_gpu_pointwise_limits.py runs the same ones on the MI355X.
Every call goes straight to the C ABI (backend(device)'s library): null outputs, one misaligned stream, hand-made strides and output
guards need that. u = 2^-53 throughout.

Guards and alignment (Buf, sweep)
    Every buffer of a call lies inside an allocation filled with the byte 0xA5, with GUARD = 64 elements of it on both sides; after the
    call the guards of every buffer are asserted unchanged. Every case runs with all streams 16-byte aligned and then once per stream with
    that stream alone at 8 mod 16 (uint8: 1 mod 16, uint16: 2 mod 16), outputs included; every configuration must return the bytes of
    the first. SMALL = 1, 2, 3, 511, 512, 513, 1025, 2559, 3072: no 512-element chunk, one, one plus an odd / even rest, 4 + 511, whole
    chunks only.

A   IEEE chains - BIT EQUALITY with oracle.hdr_oracle's float64 evaluation (every non-NaN element equal as a 64-bit pattern, signed zeros
    included; NaN positions equal). Derived, not measured: every operation is a correctly rounded IEEE + - * / sqrt, a copy or a table
    gather in the oracle's order, and both builds compile with -ffp-contract=off. hm_binary_op ADD SUB MUL DIV (value, std; stds
    ss sn ns nn), hm_compute_difference, hm_interpolate, their _bcast forms, hm_unary_op NEG, hm_u8_to_unit_f64, hm_linearize_u8 / _f64
    / _u16 (values, stds, indices), hm_gaussian_weight_u8, hm_take_axis, hm_apply_thresholds.
B   hm_pow_scalar - reference in np.longdouble from the float64 inputs: x ** p and |p x ** (p - 1)| s. Roundings counted per kind
    (k_v value, k_d the factor p x**(p-1), k_s = k_d + 3 the std: one for the product with s, 2 (k_d + 1) + 1 for its square, halved by
    the root, one for the root, rounded up):
        SQUARE  p = 2     r = x x           k_v = 1: equal to the longdouble product rounded once    d = 2 x exact      k_d = 0  k_s = 3
        ONE     p = 1     r = x             exact                                                    d = 1              k_d = 0  k_s = 3
        SQRT    p = 0.5   r = sqrt(x)       k_v = 1: equal to the longdouble root rounded once       d = .5 (1 / r)     k_d = 3  k_s = 6
                                                                                                     (root, reciprocal, product)
        INT     |p| <= 8  x ... x           k_v = |p| products (device |p| - 1; the host's pow() 1),  d = p (r / x)      k_d = k_v + 2
                                            + 1 for the reciprocal when p < 0                        (quotient, product) k_s = k_v + 5
        GENERAL libm pow  the tolerances tests/test_gpu_api.py::test_pow_scalar_exponent holds: 1e-14 on the value, 1e-13 on the std;
                          the observed maximum is recorded in units of them.
    "Rounded once": the float64 nearest the longdouble value; where that value lies within two of its own ulps of the midpoint of two
    float64s (its own rounding may have crossed it) either neighbour is accepted. A bound is (k + 2^-6) u |ref|: 2^-6 u covers the
    reference's own roundings (at most a dozen of 2^-64 each) and the second-order terms of (1 + u)^k. Asserted on every element of the benign block
    (0.05, 1.05), whose powers stay far inside [2^-1000, 2^1000]. The specials 0, -0.0, -1.5, +-inf, NaN, 5e-324, 1e-310, 1e300, 1e-300
    lie in a burst chunk, in the two-per-lane body and at the odd tail: the NaN / +-inf / +-0 pattern of value and std must be that of
    NumPy's float64 evaluation of the oracle's formula; finite non-zero results obey the bound plus one subnormal spacing (2^-1074), the
    std only where its square is a normal number (|std| >= 2^-511; below, the square under the root has lost its bits in every build).
C   libm functions - np.longdouble reference, the project's own tolerances (tests/test_gpu_api.py: RT = 1e-13 on values, 1e-12 on
    stds): hm_unary_op LOG_E (std = s / log(x) as written) and LOG_10 (std = s / (x ln10), ln10 = fl(log 5) + fl(log 2) =
    0x1.26bb1bbb55515p+1: for x = s = 1 the std must be exactly 1 / that), hm_binary_op POW. hm_gaussian_weight_f64: 1e-13 with atol
    1e-300 (tests/test_gpu_api.py::test_per_frame_kernels_many_iterations) for v in [-1.5, 2.5], where |-30 d^2| <= 120 and the three
    roundings of the argument move exp by <= 360 u = 4e-14; v = +-8 asserts only 0 <= w < 1e-300 and a finite dw. The w-only and
    dw-only calls of both weight entries must equal the two-output call bit for bit.
D   hm_binary_op's general kernel and the _bcast entries on hand-made shapes and strides (BCAST_CASES, each <= 4096 elements): six
    axes, a zero stride on the leading / an inner / the trailing axis, an outer product, size-1 axes with arbitrary strides, a strided
    slice of a larger allocation, an extent of 0 (HM_OK, nothing written), std on the broadcast operand only. Reference: the same views
    (np.lib.stride_tricks.as_strided) through the oracle, as in A (POW as in C). BAD_GEOMETRY (7 axes, 0 axes, a negative extent, a
    negative stride) is HM_EINVAL from all three entries of either build.
E   hm_apply_thresholds - C = 1..4 (k_thresholds), 5, 9, 32 (k_thresholds_wide), 33 is HM_EUNSUPPORTED; limits with +-inf and 0.0;
    values equal to a limit (kept: the comparison is strict), NaN (stays), +-inf, -0.0 against 0.0 (kept). As in A against
    oracle.apply_thresholds: every kept element keeps its bits in val and std, every clipped one is NaN in both.
F   hm_linearize_f64's index where NumPy's astype(uint8) is undefined - NaN, +-inf, |255 v| >= 2^63 - at the eight positions UNDEFINED_AT
    of n = 768 (stream kernel) and n = 383 (general kernel): the index is 0 in both builds (NaN: the convention csrc/hm_welford.hip's
    round_to_u8 cites; the others: a float64 integer of magnitude >= 2^63 is a multiple of 2^11, 0 modulo 256, and the host build answers
    0 for the infinities), and the outputs are the table's row 0. These eight elements are the only ones not compared with the oracle.
G   hm_linearize_u16 at 9, 12 and 16 bits: as in A against the oracle's gather at DN & (2^bits - 1), with and without std, lut_stride 1
    and C, stray high bits set, out_idx given and NULL.

Where this module writes a longdouble reference of its own, test_reference_is_the_oracle ties it to oracle.hdr_oracle at 1e-13. Every
check records its largest error in units of its bound or tolerance; the module prints the maxima at its end."""
import ctypes as C

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from oracle import hdr_oracle as orc

from test_stats_limits_host import LD, U, T, backend, eng, family, is_cuda, offset_by_8, record  # noqa: F401  (the shared plumbing)

WORST = {}                                                                  # family -> largest error / bound seen (this module's)
GUARD = 64
FILL = 0xA5
SMALL = [1, 2, 3, 511, 512, 513, 1025, 2559, 3072]
SPECIALS = np.array([0.0, -0.0, -1.5, np.inf, -np.inf, np.nan, 5e-324, 1e-310, 1e300, 1e-300])
RT_VAL, RT_STD = 1e-13, 1e-12                                               # tests/test_gpu_api.py: RT and the std tolerance beside it
SLACK = LD(2.0) ** -6                                                       # of u: the longdouble reference's own roundings, second-order terms
TINY = LD(2.0) ** -1074


@pytest.fixture(scope="module", autouse=True)
def report_observed_maxima():
    """After the module's tests: the largest error of each family in units of its bound (DESIGN.md section 5 quotes them)."""
    yield
    print("\nobserved maxima, in units of the bound:", {k: round(v, 4) for k, v in sorted(WORST.items())})


def rec(fam, err, bound):
    worst = record(fam, err, bound)
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    return worst


# ------------------------------------------------------------------------------------------------ guarded buffers
class Buf:
    """n elements of `dtype` at `mis` bytes past a 16-byte boundary, GUARD elements of FILL bytes on both sides."""

    def __init__(self, device, dtype, n, mis=0, init=None):
        self.dtype, self.n = np.dtype(dtype), int(n)
        item = self.dtype.itemsize
        self.nbytes = self.n * item
        self.raw = torch.full((self.nbytes + 2 * GUARD * item + 32,), FILL, dtype=torch.uint8, device=device)
        self.start = GUARD * item
        self.start += (mis - (self.raw.data_ptr() + self.start)) % 16
        self.ptr = self.raw.data_ptr() + self.start
        assert self.ptr % 16 == mis % 16 and self.ptr % item == 0
        if init is not None:
            init = np.ascontiguousarray(init, self.dtype).ravel()
            assert init.size == self.n
            if self.n:
                self.raw[self.start:self.start + self.nbytes].copy_(torch.from_numpy(init.view(np.uint8).copy()))

    def get(self, what=""):
        """-> the n elements; asserts both guards untouched."""
        host = self.raw.cpu().numpy()
        assert np.all(host[:self.start] == FILL), f"{what}: written before the buffer"
        assert np.all(host[self.start + self.nbytes:] == FILL), f"{what}: written past the buffer"
        return host[self.start:self.start + self.nbytes].copy().view(self.dtype)


def mis_of(dtype):
    return {8: 8, 1: 1, 2: 2}[np.dtype(dtype).itemsize]


def sweep(device, streams, call, what, configs=None, inplace=()):
    """streams: [(name, dtype, n, init or None (an output), or None for a NULL stream)]. call(lib, stream, {name: ptr or None}) -> status.
    Runs all-aligned, then each stream alone misaligned; returns the outputs {name: array} of the aligned run after asserting that
    every configuration returned the same bytes (outputs: the streams without init, and those named in `inplace`)."""
    live = [i for i, s in enumerate(streams) if s is not None]
    configs = [None] + live if configs is None else configs
    first = None
    for off in configs:
        with backend(device) as (lib, stream):
            bufs = {}
            for i, s in enumerate(streams):
                if s is None:
                    continue
                name, dtype, n, init = s
                bufs[name] = Buf(device, dtype, n, mis_of(dtype) if off == i else 0, init)
            rc = call(lib, stream, {s[0]: bufs[s[0]].ptr for s in streams if s is not None})
            assert rc == nat.HM_OK, f"{what}: status {rc} with stream {off} offset"
            if is_cuda(device):
                torch.cuda.synchronize()
            got = {s[0]: bufs[s[0]].get(f"{what}, stream {off} offset: {s[0]}") for s in streams          # the outputs (and their guards)
                   if s is not None and (s[3] is None or s[0] in inplace)}
        if first is None:
            first = got
        else:
            for name in got:
                assert np.array_equal(got[name].view(np.uint8), first[name].view(np.uint8)), \
                    f"{what}: {name} differs when stream {streams[off][0]} alone is misaligned"
    return first


def assert_bits(got, ref, what):
    got = np.ascontiguousarray(got, np.float64).ravel()
    ref = np.ascontiguousarray(ref, np.float64).ravel()
    assert got.shape == ref.shape, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ at {np.flatnonzero(np.isnan(got) != nan)[:6]}"
    bad = (got.view(np.uint64) != ref.view(np.uint64)) & ~nan
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ, first at {np.flatnonzero(bad)[:6]}: {got[bad][:3]!r} != {ref[bad][:3]!r}"


def assert_close(fam, got, ref_ld, rtol, what, atol=0.0):
    """|got - ref| <= rtol |ref| + atol on the finite elements of the longdouble reference, the non-finite pattern equal."""
    got = np.asarray(got, np.float64).ravel()
    ref_ld = np.asarray(ref_ld, LD).ravel()
    with np.errstate(all="ignore"):
        r64 = ref_ld.astype(np.float64)
    fin = np.isfinite(r64)
    assert np.array_equal(np.isnan(got), np.isnan(r64)) and np.array_equal(got[~fin & ~np.isnan(r64)], r64[~fin & ~np.isnan(r64)]), f"{what}: non-finite pattern"
    if fin.any():
        worst = rec(fam, np.abs(got[fin].astype(LD) - ref_ld[fin]), LD(rtol) * np.abs(ref_ld[fin]) + LD(atol) + TINY)
        assert worst <= 1.0, f"{what}: {worst:.3f} x the tolerance {rtol}"


def values(rng, n, specials=True):
    x = 0.05 + rng.random(n)
    if specials and n >= 3:
        at = rng.integers(0, n, max(1, n // 37))
        x[at] = rng.choice(SPECIALS, at.size)
    return x


def stds(rng, n):
    s = 0.01 + 0.05 * rng.random(n)
    if n >= 3:
        s[rng.integers(0, n, max(1, n // 61))] = 0.0
    return s


def i64(seq):
    return (C.c_int64 * len(seq))(*[int(v) for v in seq])


def f64(seq):
    return (C.c_double * len(seq))(*[float(v) for v in seq])


# ------------------------------------------------------------------------------------------------ A: binary, difference, interpolate
OPS = {nat_op: fn for nat_op, fn in zip(range(5), (orc.op_add, orc.op_sub, orc.op_mul, orc.op_div, orc.op_pow))}
OP_NAMES = ["add", "sub", "mul", "div", "pow"]
STD_COMBOS = [(True, True), (True, False), (False, True), (False, False)]
MULT, Y0, Y1, Y = 1.7, 0.25, 2.0, 0.9


def dense_inputs(n, seed, specials=True):
    rng = np.random.default_rng(seed)
    return values(rng, n, specials), stds(rng, n), values(rng, n, specials), stds(rng, n)


def run_binary_dense(device, op, n, std1, std2, x1, s1, x2, s2, configs=None):
    streams = [("x1", np.float64, n, x1), ("s1", np.float64, n, s1) if std1 else None, ("x2", np.float64, n, x2),
               ("s2", np.float64, n, s2) if std2 else None, ("out", np.float64, n, None),
               ("out_std", np.float64, n, None) if std1 or std2 else None]

    def call(lib, stream, p):
        return lib.hm_binary_op(op, p["x1"], p.get("s1"), p["x2"], p.get("s2"), p["out"], p.get("out_std"), 1, i64([n]), i64([1]), i64([1]), stream)
    return sweep(device, streams, call, f"hm_binary_op {OP_NAMES[op]} n={n} std={std1, std2}", configs)


def check_binary_dense(device, op, sizes=SMALL):
    """ADD / SUB / MUL / DIV on dense operands (burst, two-per-lane and strided kernels by size and alignment): bit equality."""
    for n in sizes:
        x1, s1, x2, s2 = dense_inputs(n, 100 * op + n)
        for std1, std2 in STD_COMBOS:
            got = run_binary_dense(device, op, n, std1, std2, x1, s1, x2, s2)
            with np.errstate(all="ignore"):
                rv, rs = OPS[op](x1, s1 if std1 else None, x2, s2 if std2 else None)
            what = f"{OP_NAMES[op]} n={n} std={std1, std2}"
            assert_bits(got["out"], rv, what + " value")
            if std1 or std2:
                assert_bits(got["out_std"], rs, what + " std")


def run_difference(device, n, sx_, sy_, x, sx, y, sy, configs=None):
    with_std = sx_ or sy_
    streams = [("x", np.float64, n, x), ("sx", np.float64, n, sx) if sx_ else None, ("y", np.float64, n, y), ("sy", np.float64, n, sy) if sy_ else None,
               ("ad", np.float64, n, None), ("ads", np.float64, n, None) if with_std else None, ("rd", np.float64, n, None),
               ("rds", np.float64, n, None) if with_std else None]

    def call(lib, stream, p):
        return lib.hm_compute_difference(p["x"], p.get("sx"), p["y"], p.get("sy"), MULT, p["ad"], p.get("ads"), p["rd"], p.get("rds"), n, stream)
    return sweep(device, streams, call, f"hm_compute_difference n={n} std={sx_, sy_}", configs)


def assert_difference(got, x, sx, y, sy, what):
    with np.errstate(all="ignore"):
        a, as_, r, rs = orc.compute_difference(x, sx, y, sy, MULT)
    assert_bits(got["ad"], a, what + " abs")
    assert_bits(got["rd"], r, what + " rel")
    if sx is not None or sy is not None:
        assert_bits(got["ads"], np.broadcast_to(as_, a.shape), what + " abs std")
        assert_bits(got["rds"], rs, what + " rel std")


def check_difference(device, sizes=SMALL):
    for n in sizes:
        x, sx, y, sy = dense_inputs(n, 7000 + n)
        for a, b in STD_COMBOS:
            got = run_difference(device, n, a, b, x, sx, y, sy)
            assert_difference(got, x, sx if a else None, y, sy if b else None, f"difference n={n} std={a, b}")


def run_interpolate(device, n, a_, b_, x0, s0, x1, s1, configs=None):
    streams = [("x0", np.float64, n, x0), ("s0", np.float64, n, s0) if a_ else None, ("x1", np.float64, n, x1), ("s1", np.float64, n, s1) if b_ else None,
               ("out", np.float64, n, None), ("out_std", np.float64, n, None) if a_ or b_ else None]

    def call(lib, stream, p):
        return lib.hm_interpolate(p["x0"], p.get("s0"), p["x1"], p.get("s1"), Y0, Y1, Y, p["out"], p.get("out_std"), n, stream)
    return sweep(device, streams, call, f"hm_interpolate n={n} std={a_, b_}", configs)


def assert_interpolate(got, x0, s0, x1, s1, what):
    with np.errstate(all="ignore"):
        rv, rs = orc.interpolate(x0, s0, x1, s1, Y0, Y1, Y)
    assert_bits(got["out"], rv, what + " value")
    if rs is not None:
        assert_bits(got["out_std"], rs, what + " std")


def check_interpolate(device, sizes=SMALL):
    for n in sizes:
        x0, s0, x1, s1 = dense_inputs(n, 9000 + n)
        for a, b in STD_COMBOS:
            got = run_interpolate(device, n, a, b, x0, s0, x1, s1)
            assert_interpolate(got, x0, s0 if a else None, x1, s1 if b else None, f"interpolate n={n} std={a, b}")


# ------------------------------------------------------------------------------------------------ A / C: unary
def run_unary(device, op, n, x, s, configs=None):
    streams = [("x", np.float64, n, x), ("s", np.float64, n, s) if s is not None else None, ("out", np.float64, n, None),
               ("out_std", np.float64, n, None) if s is not None else None]

    def call(lib, stream, p):
        return lib.hm_unary_op(op, p["x"], p.get("s"), p["out"], p.get("out_std"), n, stream)
    return sweep(device, streams, call, f"hm_unary_op {op} n={n}", configs)


def log_reference(x, s, base10):
    """longdouble: log / log10 and the reference's std formulas (measurand.py:258 as written, :277)."""
    xl, sl_ = x.astype(LD), s.astype(LD)
    if base10:
        return np.log10(xl), sl_ / (xl * (np.log(LD(5)) + np.log(LD(2))))
    return np.log(xl), sl_ / np.log(xl)


def log_inputs(n, seed):
    rng = np.random.default_rng(seed)
    x = np.where(rng.random(n) < 0.5, 0.05 + 0.85 * rng.random(n), 1.1 + 9 * rng.random(n))       # away from log(x) = 0, where s / log(x) has no scale
    return x, 0.01 + 0.05 * rng.random(n)


def check_unary(device, sizes=SMALL):
    for n in sizes:
        rng = np.random.default_rng(300 + n)
        x, s = values(rng, n), stds(rng, n)
        for with_std in (True, False):
            got = run_unary(device, 0, n, x, s if with_std else None)
            assert_bits(got["out"], orc.op_neg(x, None)[0], f"neg n={n}")
            if with_std:
                assert_bits(got["out_std"], s, f"neg std n={n}")
        x, s = log_inputs(n, 400 + n)
        for op, base10 in ((1, False), (2, True)):
            fam = family(device, "log_10" if base10 else "log_e")
            got = run_unary(device, op, n, x, s)
            rv, rs = log_reference(x, s, base10)
            assert_close(fam + " value", got["out"], rv, RT_VAL, f"log op {op} n={n}")
            assert_close(fam + " std", got["out_std"], rs, RT_STD, f"log op {op} std n={n}")
            only = run_unary(device, op, n, x, None, configs=[None])
            assert_bits(only["out"], got["out"], f"log op {op} n={n} without std")


LN10 = float.fromhex("0x1.26bb1bbb55515p+1")                                 # fl(log 5) + fl(log 2), measurand.py:277


def check_log10_constant(device):
    """x = s = 1: the std is 1 / ln10 with the reference's constant, exactly."""
    assert np.log(5.0) + np.log(2.0) == LN10
    for n in (1, 2, 600):
        got = run_unary(device, 2, n, np.ones(n), np.ones(n), configs=[None])
        assert_bits(got["out_std"], np.full(n, 1.0 / LN10), "log_10 std at x = s = 1")
        assert_bits(got["out"], np.zeros(n), "log_10(1)")


# ------------------------------------------------------------------------------------------------ B: pow with a scalar exponent
INT_EXPONENTS = [p for p in range(-8, 9) if p != 0]
EXPONENTS = [2.0, 0.5, 1.0] + [float(p) for p in INT_EXPONENTS if p not in (1, 2)] + [0.0, 9.0, -9.0, 2.5, -0.75, float(np.nextafter(8.0, np.inf))]
ODD_EXPONENTS = [np.nan, np.inf, -np.inf]
SWEPT_EXPONENTS = [2.0, 0.5, 1.0, -3.0, 2.5]                                 # one of each kind gets the one-stream-misaligned sweep


def pow_kind(p):
    if p == 2.0:
        return "square"
    if p == 0.5:
        return "sqrt"
    if p == 1.0:
        return "one"
    if np.isfinite(p) and p == int(p) and 1 <= abs(p) <= 8:
        return "int"
    return "general"


def pow_counts(p):
    """-> (k_v, k_s): roundings of the value and of the std, the module docstring's table."""
    kind = pow_kind(p)
    if kind == "general":
        return 0, 0                                                         # (tolerances, not counts)
    if kind in ("square", "one"):
        return 1, 3
    if kind == "sqrt":
        return 1, 6
    k_v = int(abs(p)) + (1 if p < 0 else 0)
    return k_v, k_v + 5


def ld_power(xl, q):
    """xl ** q in longdouble: products (and a reciprocal) for an integer |q| <= 9, the root for +-0.5, powl otherwise."""
    if np.isfinite(q) and q == int(q) and abs(q) <= 9:
        r = np.ones_like(xl)
        for _ in range(int(abs(q))):
            r = r * xl
        return 1 / r if q < 0 else r
    if abs(q) == 0.5:
        return np.sqrt(xl) if q > 0 else 1 / np.sqrt(xl)
    return xl ** LD(q)


def pow_reference(x, s, p):
    """longdouble x ** p and |p x ** (p - 1)| s from the float64 inputs."""
    with np.errstate(all="ignore"):
        xl = x.astype(LD)
        return ld_power(xl, p), np.abs(LD(p) * ld_power(xl, p - 1.0)) * s.astype(LD)


def round_once(ref_ld):
    """-> (the float64 nearest ref_ld, a mask of the elements within two longdouble ulps of a float64 midpoint)."""
    r = ref_ld.astype(np.float64)
    half = np.abs(np.spacing(r)).astype(LD) / 2
    dist = np.abs(ref_ld - r.astype(LD))
    return r, np.abs(dist - half) <= 2 * np.abs(np.spacing(ref_ld))


def assert_rounded_once(got, ref_ld, what):
    r, amb = round_once(ref_ld)
    ok = got.view(np.uint64) == r.view(np.uint64)
    ok |= amb & ((got == np.nextafter(r, -np.inf)) | (got == np.nextafter(r, np.inf)))
    assert ok.all(), f"{what}: not the correctly rounded value at {np.flatnonzero(~ok)[:6]}: {got[~ok][:3]!r} != {r[~ok][:3]!r}"


def assert_pow_benign(device, p, x, s, gv, gs, what):
    rv, rs = pow_reference(x, s, p)
    kind, (k_v, k_s) = pow_kind(p), pow_counts(p)
    fam = family(device, f"pow_scalar {kind}")
    if kind == "one":
        assert_bits(gv, x, what + " value")
    elif kind in ("square", "sqrt"):
        assert_rounded_once(gv, rv, what + " value")
    elif kind == "int":
        worst = rec(fam + " value", np.abs(gv.astype(LD) - rv), (k_v + SLACK) * LD(U) * np.abs(rv))
        assert worst <= 1.0, f"{what}: value {worst:.3f} x the bound {k_v} u"
    else:
        assert_close(fam + " value", gv, rv, 1e-14, what + " value")
    if gs is not None:
        if kind == "general":
            assert_close(fam + " std", gs, rs, 1e-13, what + " std")
        else:
            worst = rec(fam + " std", np.abs(gs.astype(LD) - rs), (k_s + SLACK) * LD(U) * np.abs(rs) + TINY)
            assert worst <= 1.0, f"{what}: std {worst:.3f} x the bound {k_s} u"


def numpy_pow(x, s, p):
    """NumPy's float64 evaluation of the oracle's formula: the pattern of zeros, infinities and NaNs the specials must show."""
    with np.errstate(all="ignore"):
        return orc.op_pow(x, s, np.array([float(p)]), None)


def same_class(got, ref, what):
    """NaN positions, +-inf and +-0 equal."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern: got {got!r}, NumPy {ref!r}"
    for probe in (np.isposinf, np.isneginf):
        assert np.array_equal(probe(got), probe(ref)), f"{what}: inf pattern: got {got!r}, NumPy {ref!r}"
    z = (ref == 0)
    assert np.array_equal(got == 0, z) and np.array_equal(np.signbit(got[z]), np.signbit(ref[z])), f"{what}: zero pattern: got {got!r}, NumPy {ref!r}"


def assert_pow_specials(device, p, x, s, gv, gs, what):
    nv, ns = numpy_pow(x, s, p)
    same_class(gv, nv, what + " value")
    kind, (k_v, k_s) = pow_kind(p), pow_counts(p)
    if not np.isfinite(p):
        if gs is not None:
            assert np.array_equal(np.isnan(gs), np.isnan(ns)) and np.array_equal(np.isinf(gs), np.isinf(ns)), f"{what} std: got {gs!r}, NumPy {ns!r}"
        return
    rv, rs = pow_reference(x, s, p)
    rel_v, rel_s = ((1e-14 / U, 1e-13 / U) if kind == "general" else (k_v, k_s))
    fin = np.isfinite(nv) & (nv != 0)
    fam = family(device, "pow_scalar specials")
    if fin.any():
        worst = rec(fam, np.abs(gv[fin].astype(LD) - rv[fin]), (rel_v + SLACK) * LD(U) * np.abs(rv[fin]) + TINY)
        assert worst <= 1.0, f"{what}: special values {worst:.3f} x the bound: got {gv[fin]!r}"
    if gs is not None:
        same_class(gs, ns, what + " std")
        fin = np.isfinite(ns) & (np.abs(ns) >= 2.0 ** -511)
        if fin.any():
            worst = rec(fam, np.abs(gs[fin].astype(LD) - rs[fin]), (rel_s + SLACK) * LD(U) * np.abs(rs[fin]) + TINY)
            assert worst <= 1.0, f"{what}: special stds {worst:.3f} x the bound: got {gs[fin]!r}"


def run_pow(device, p, n, x, s, configs=None):
    streams = [("x", np.float64, n, x), ("s", np.float64, n, s) if s is not None else None, ("out", np.float64, n, None),
               ("out_std", np.float64, n, None) if s is not None else None]

    def call(lib, stream, q):
        return lib.hm_pow_scalar(q["x"], q.get("s"), float(p), q["out"], q.get("out_std"), n, stream)
    return sweep(device, streams, call, f"hm_pow_scalar p={p} n={n}", configs)


def check_pow_benign(device, p, sizes=SMALL):
    """The bound on every element of the benign block, at every small size: burst chunks, the two-per-lane body aligned and (one stream
    offset) unaligned, the odd tail; with and without std."""
    for n in sizes:
        rng = np.random.default_rng(int(1000 * abs(p)) % 9973 + n)
        x, s = 0.05 + rng.random(n), 0.01 + 0.05 * rng.random(n)
        configs = None if p in SWEPT_EXPONENTS else [None, 2]
        got = run_pow(device, p, n, x, s, configs)
        assert_pow_benign(device, p, x, s, got["out"], got["out_std"], f"pow_scalar p={p} n={n}")
        only = run_pow(device, p, n, x, None, None if p in SWEPT_EXPONENTS else [None, 0])
        assert_bits(only["out"], got["out"], f"pow_scalar p={p} n={n} without std")


SPECIALS_N = 553                                                            # one chunk, 20 pairs, one odd element
SPECIALS_AT = (100, 520)                                                    # a burst chunk; the two-per-lane body


def special_inputs(p_index):
    rng = np.random.default_rng(555)
    x, s = 0.05 + rng.random(SPECIALS_N), 0.01 + 0.05 * rng.random(SPECIALS_N)
    for at in SPECIALS_AT:
        x[at:at + SPECIALS.size] = SPECIALS
    x[-1] = SPECIALS[p_index % SPECIALS.size]                               # the odd tail
    where = np.r_[SPECIALS_AT[0]:SPECIALS_AT[0] + SPECIALS.size, SPECIALS_AT[1]:SPECIALS_AT[1] + SPECIALS.size, SPECIALS_N - 1]
    return x, s, where


def check_pow_specials(device, p_index, p):
    x, s, where = special_inputs(p_index)
    benign = np.setdiff1d(np.arange(SPECIALS_N), where)
    for with_std in (True, False):
        got = run_pow(device, p, SPECIALS_N, x, s if with_std else None, configs=[None, 0])
        gv, gs = got["out"], got.get("out_std")
        what = f"pow_scalar p={p} specials std={with_std}"
        assert_pow_specials(device, p, x[where], s[where], gv[where], None if gs is None else gs[where], what)
        if np.isfinite(p):
            assert_pow_benign(device, p, x[benign], s[benign], gv[benign], None if gs is None else gs[benign], what + " (benign part)")


def check_pow_tail_specials(device, p):
    """n = 3: every special in turn as the odd tail element, and n = 1."""
    for k, v in enumerate(SPECIALS):
        for n in (3, 1):
            x, s = np.full(n, 0.7), np.full(n, 0.03)
            x[-1] = v
            got = run_pow(device, p, n, x, s, configs=[None])
            assert_pow_specials(device, p, x, s, got["out"], got["out_std"], f"pow_scalar p={p} tail special {v!r} n={n}")


def check_pow_half_at_numpy(device):
    """x ** 0.5 at -inf and -0.0: NumPy's own answers (+inf, +0.0; the factor x ** -0.5: +0, +inf), sqrt's everywhere else."""
    x = np.array([-np.inf, -0.0, 0.0, np.inf, -1.5])
    with np.errstate(all="ignore"):
        assert_bits(x ** np.array([0.5]), [np.inf, 0.0, 0.0, np.inf, np.nan], "NumPy's x ** 0.5")
        assert_bits(x ** np.array([-0.5]), [0.0, np.inf, np.inf, 0.0, np.nan], "NumPy's x ** -0.5")
    for n, pad in ((5, 0), (517, 512)):                                     # two-per-lane + tail; one burst chunk in front
        xx = np.r_[np.full(pad, 0.25), x]
        got = run_pow(device, 0.5, n, xx, np.ones(n), configs=[None])
        assert_bits(got["out"][pad:], [np.inf, 0.0, 0.0, np.inf, np.nan], f"x ** 0.5 n={n}")
        assert_bits(got["out"][:pad], np.full(pad, 0.5), f"x ** 0.5 n={n}")
        assert np.isnan(got["out_std"][pad:]).all()                         # (log(x) x**p) * 0 is NaN for every x <= 0 and for +inf
        only = run_pow(device, 0.5, n, xx, None, configs=[None])
        assert_bits(only["out"], got["out"], "x ** 0.5 without std")


# ------------------------------------------------------------------------------------------------ C: pow with an array exponent, weights
def binary_pow_reference(x1, s1, x2, s2):
    a, b = x1.astype(LD), x2.astype(LD)
    r = a ** b
    if s1 is None and s2 is None:
        return r, None
    z1 = np.zeros_like(a) if s1 is None else s1.astype(LD)
    z2 = np.zeros_like(a) if s2 is None else s2.astype(LD)
    return r, np.sqrt(((b * a ** (b - 1)) * z1) ** 2 + ((np.log(a) * r) * z2) ** 2)


def check_binary_pow(device, sizes=SMALL):
    fam = family(device, "binary pow")
    for n in sizes:
        rng = np.random.default_rng(5000 + n)
        x1, s1, x2, s2 = 0.05 + rng.random(n), stds(rng, n), 6 * rng.random(n) - 3, stds(rng, n)
        for a, b in STD_COMBOS:
            got = run_binary_dense(device, 4, n, a, b, x1, s1, x2, s2, configs=[None, 0])
            rv, rs = binary_pow_reference(x1, s1 if a else None, x2, s2 if b else None)
            assert_close(fam + " value", got["out"], rv, RT_VAL, f"pow n={n} std={a, b}")
            if rs is not None:
                assert_close(fam + " std", got["out_std"], rs, RT_STD, f"pow n={n} std={a, b} std")


def run_weight_f64(device, n, v, want_w, want_dw, configs=None):
    streams = [("v", np.float64, n, v), ("w", np.float64, n, None) if want_w else None, ("dw", np.float64, n, None) if want_dw else None]

    def call(lib, stream, p):
        return lib.hm_gaussian_weight_f64(p["v"], p.get("w"), p.get("dw"), n, stream)
    return sweep(device, streams, call, f"hm_gaussian_weight_f64 n={n} outputs={want_w, want_dw}", configs)


def weight_reference(v):
    d = v.astype(LD) - LD(0.5)
    w = np.exp(LD(-30) * d * d)
    return w, LD(-60) * d * w


def check_weight_f64(device, sizes=SMALL):
    fam = family(device, "gaussian weight")
    for n in sizes:
        v = -1.5 + 4.0 * np.random.default_rng(600 + n).random(n)
        both = run_weight_f64(device, n, v, True, True)
        rw, rdw = weight_reference(v)
        assert_close(fam + " w", both["w"], rw, 1e-13, f"weight n={n}", atol=1e-300)
        assert_close(fam + " dw", both["dw"], rdw, 1e-13, f"weight dw n={n}", atol=1e-300)
        assert_bits(run_weight_f64(device, n, v, True, False)["w"], both["w"], f"weight n={n}: w alone")
        assert_bits(run_weight_f64(device, n, v, False, True)["dw"], both["dw"], f"weight n={n}: dw alone")
    far = np.tile([8.0, -8.0, -7.0], 200)
    got = run_weight_f64(device, far.size, far, True, True, configs=[None])
    assert np.all((got["w"] >= 0) & (got["w"] < 1e-300)) and np.isfinite(got["dw"]).all()


def run_weight_u8(device, n, dn, luts, want_w, want_dw, configs=None):
    streams = [("dn", np.uint8, n, dn), ("wl", np.float64, 256, luts[0]), ("dwl", np.float64, 256, luts[1]),
               ("w", np.float64, n, None) if want_w else None, ("dw", np.float64, n, None) if want_dw else None]

    def call(lib, stream, p):
        return lib.hm_gaussian_weight_u8(p["dn"], p["wl"], p["dwl"], p.get("w"), p.get("dw"), n, stream)
    configs = [None, 0, 3, 4] if configs is None else configs               # the tables are read element by element: not swept
    return sweep(device, streams, call, f"hm_gaussian_weight_u8 n={n} outputs={want_w, want_dw}",
                 [c for c in configs if c is None or streams[c] is not None])


def check_weight_u8(device, sizes=SMALL):
    luts = orc.gaussian_weight_lut()
    for n in sizes:
        dn = np.random.default_rng(700 + n).integers(0, 256, n).astype(np.uint8)
        dn[:2] = (0, 255)[:min(n, 2)]
        both = run_weight_u8(device, n, dn, luts, True, True)
        assert_bits(both["w"], luts[0][dn], f"weight u8 n={n}")
        assert_bits(both["dw"], luts[1][dn], f"weight u8 dw n={n}")
        assert_bits(run_weight_u8(device, n, dn, luts, True, False)["w"], both["w"], f"weight u8 n={n}: w alone")
        assert_bits(run_weight_u8(device, n, dn, luts, False, True)["dw"], both["dw"], f"weight u8 n={n}: dw alone")


# ------------------------------------------------------------------------------------------------ A: u8 -> unit, take
def check_u8_to_unit(device, sizes=SMALL):
    for n in sizes:
        dn = np.random.default_rng(800 + n).integers(0, 256, n).astype(np.uint8)

        def call(lib, stream, p):
            return lib.hm_u8_to_unit_f64(p["dn"], p["out"], n, stream)
        got = sweep(device, [("dn", np.uint8, n, dn), ("out", np.float64, n, None)], call, f"hm_u8_to_unit_f64 n={n}")
        assert_bits(got["out"], orc.unit_from_u8(dn), f"u8_to_unit n={n}")


TAKE_CASES = [((1, 5, 1), [0]), ((1, 7, 1), [6, -7, 3]), ((3, 4, 5), [-1, 0, 0, 2]), ((17, 3, 31), [2, 1]), ((2, 16, 9), list(range(15, -1, -1))),
              ((1, 2, 513), [1, 0, 1])]


def run_take(device, shape, idx, x, s, configs=None):
    outer, axis_len, inner = shape
    n_in, n_out = outer * axis_len * inner, outer * len(idx) * inner
    streams = [("x", np.float64, n_in, x), ("s", np.float64, n_in, s) if s is not None else None, ("out", np.float64, n_out, None),
               ("out_std", np.float64, n_out, None) if s is not None else None]

    def call(lib, stream, p):
        return lib.hm_take_axis(p["x"], p.get("s"), p["out"], p.get("out_std"), outer, axis_len, inner, i64(idx), len(idx), stream)
    return sweep(device, streams, call, f"hm_take_axis {shape} {idx}", configs)


def check_take(device, cases=TAKE_CASES):
    for shape, idx in cases:
        rng = np.random.default_rng(sum(shape))
        x, s = values(rng, int(np.prod(shape))).reshape(shape), stds(rng, int(np.prod(shape))).reshape(shape)
        for with_std in (True, False):
            got = run_take(device, shape, idx, x, s if with_std else None)
            assert_bits(got["out"], np.take(x, idx, axis=1), f"take {shape} {idx}")
            if with_std:
                assert_bits(got["out_std"], np.take(s, idx, axis=1), f"take std {shape} {idx}")
    with backend(device) as (lib, stream):                                  # an index out of range, before anything is written
        b = Buf(device, np.float64, 8, 0, np.zeros(8))
        o = Buf(device, np.float64, 8)
        for bad in ([4], [-5]):
            assert lib.hm_take_axis(b.ptr, None, o.ptr, None, 2, 4, 1, i64(bad), 1, stream) == nat.HM_ESHAPE
        assert np.all(o.get("take, bad index").view(np.uint8) == FILL)


# ------------------------------------------------------------------------------------------------ D: hand-made shapes and strides
def strided(base, shape, strides, offset=0):
    """The view of the 1-D float64 `base` with the given ELEMENT strides."""
    return np.lib.stride_tricks.as_strided(base[offset:], shape, [8 * st for st in strides], writeable=False)


def span(shape, strides):
    return 1 + sum((n - 1) * st for n, st in zip(shape, strides)) if all(n > 0 for n in shape) else 1


# name, shape, strides of operand 1, strides of operand 2
BCAST_CASES = [
    ("six axes", (2, 3, 2, 3, 2, 5), (180, 60, 30, 10, 5, 1), (30, 0, 15, 5, 0, 1)),
    ("leading axis broadcast", (7, 33), (33, 1), (0, 1)),
    ("inner axis broadcast", (5, 4, 31), (124, 31, 1), (31, 0, 1)),
    ("trailing axis broadcast", (40, 9), (9, 1), (1, 0)),
    ("outer product", (37, 29), (1, 0), (0, 1)),
    ("size-1 axes, arbitrary strides", (1, 50, 1), (12345, 1, 777), (99, 1, 5)),
    ("strided slice", (32, 20), (140, 3), (1, 0)),
    ("both strided, three chunks", (3, 600), (1300, 2), (0, 3)),
    ("extent 0", (4, 0, 3), (0, 3, 1), (0, 3, 1)),
]
BAD_GEOMETRY = [("seven axes", (1,) * 7, (1,) * 7, (1,) * 7), ("no axes", (), (), ()), ("negative extent", (4, -2), (2, 1), (2, 1)),
                ("negative stride, operand 1", (4, 2), (2, -1), (2, 1)), ("negative stride, operand 2", (4, 2), (2, 1), (-2, 1))]
BCAST_STDS = [(True, True), (False, True), (True, False), (False, False)]   # (False, True): std on the broadcast operand only


def bcast_operands(case, seed):
    name, shape, st1, st2 = case
    rng = np.random.default_rng(seed)
    n1, n2 = span(shape, st1), span(shape, st2)
    return values(rng, n1), stds(rng, n1), values(rng, n2), stds(rng, n2)


def run_bcast(device, entry, case, std1, std2, ops, op=None):
    """entry: 'binary' (op), 'difference', 'interpolate' -> {name: flat array} of the dense outputs."""
    name, shape, st1, st2 = case
    b1, e1, b2, e2 = ops
    n = int(np.prod(shape))
    with_std = std1 or std2
    ins = [("x1", np.float64, b1.size, b1), ("s1", np.float64, b1.size, e1) if std1 else None, ("x2", np.float64, b2.size, b2),
           ("s2", np.float64, b2.size, e2) if std2 else None]
    outs = {"binary": ["out", "out_std"], "interpolate": ["out", "out_std"], "difference": ["ad", "ads", "rd", "rds"]}[entry]
    streams = ins + [(o, np.float64, n, None) if (with_std or not o.endswith(("std", "s"))) else None for o in outs]
    geometry = (len(shape), i64(shape), i64(st1), i64(st2))

    def call(lib, stream, p):
        if entry == "binary":
            return lib.hm_binary_op(op, p["x1"], p.get("s1"), p["x2"], p.get("s2"), p["out"], p.get("out_std"), *geometry, stream)
        if entry == "difference":
            return lib.hm_compute_difference_bcast(p["x1"], p.get("s1"), p["x2"], p.get("s2"), MULT, p["ad"], p.get("ads"), p["rd"], p.get("rds"), *geometry, stream)
        return lib.hm_interpolate_bcast(p["x1"], p.get("s1"), p["x2"], p.get("s2"), Y0, Y1, Y, p["out"], p.get("out_std"), *geometry, stream)
    return sweep(device, streams, call, f"{entry} {op} on '{name}' std={std1, std2}", configs=[None, 0, len(ins)])


def check_bcast(device, entry, op=None, cases=BCAST_CASES):
    for k, case in enumerate(cases):
        name, shape, st1, st2 = case
        ops = bcast_operands(case, 40 + k)
        if op == 4:                                                         # pow: a positive base, exponents in (-3, 3)
            rng = np.random.default_rng(k)
            ops = (0.05 + rng.random(ops[0].size), ops[1], 6 * rng.random(ops[2].size) - 3, ops[3])
        v1, u1, v2, u2 = (strided(a, shape, st) for a, st in zip(ops, (st1, st1, st2, st2)))
        for std1, std2 in BCAST_STDS:
            got = run_bcast(device, entry, case, std1, std2, ops, op)
            what = f"{entry} {op} on '{name}' std={std1, std2}"
            if 0 in shape:
                assert got and all(g.size == 0 for g in got.values())
                continue
            a, b = (u1 if std1 else None), (u2 if std2 else None)
            if entry == "difference":
                assert_difference(got, v1, a, v2, b, what)
            elif entry == "interpolate":
                assert_interpolate(got, v1, a, v2, b, what)
            elif op == 4:
                rv, rs = binary_pow_reference(np.ascontiguousarray(v1), None if a is None else np.ascontiguousarray(a), np.ascontiguousarray(v2),
                                              None if b is None else np.ascontiguousarray(b))
                assert_close(family(device, "binary pow") + " value", got["out"], rv, RT_VAL, what)
                if rs is not None:
                    assert_close(family(device, "binary pow") + " std", got["out_std"], rs, RT_STD, what + " std")
            else:
                with np.errstate(all="ignore"):
                    rv, rs = OPS[op](v1, a, v2, b)
                assert_bits(got["out"], rv, what + " value")
                if rs is not None:
                    assert_bits(got["out_std"], rs, what + " std")


def bad_geometry_statuses(device):
    """-> {(entry, case name): status}: nothing may be written (outputs are guards only) and nothing read."""
    out = {}
    with backend(device) as (lib, stream):
        x = Buf(device, np.float64, 64, 0, np.ones(64))
        o = [Buf(device, np.float64, 64) for _ in range(4)]
        for name, shape, st1, st2 in BAD_GEOMETRY:
            g = (len(shape), i64(shape), i64(st1), i64(st2))
            out["binary", name] = lib.hm_binary_op(0, x.ptr, x.ptr, x.ptr, x.ptr, o[0].ptr, o[1].ptr, *g, stream)
            out["difference", name] = lib.hm_compute_difference_bcast(x.ptr, x.ptr, x.ptr, x.ptr, MULT, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, *g, stream)
            out["interpolate", name] = lib.hm_interpolate_bcast(x.ptr, x.ptr, x.ptr, x.ptr, Y0, Y1, Y, o[0].ptr, o[1].ptr, *g, stream)
        out["binary", "unknown op"] = lib.hm_binary_op(5, x.ptr, None, x.ptr, None, o[0].ptr, None, 1, i64([4]), i64([1]), i64([1]), stream)
        if is_cuda(device):
            torch.cuda.synchronize()
        for b in o:
            assert np.all(b.get("refused geometry").view(np.uint8) == FILL)
    return out


def check_bad_geometry(device):
    got = bad_geometry_statuses(device)
    assert got and all(rc == nat.HM_EINVAL for rc in got.values()), {k: v for k, v in got.items() if v != nat.HM_EINVAL}


# ------------------------------------------------------------------------------------------------ E: thresholds
THRESHOLD_CHANNELS = [1, 2, 3, 4, 5, 9, 32]


def by_channel(flat, C_, fn):
    """fn on the (rows, C) view of `flat` padded to whole rows -> flat results cut back to flat.size."""
    n = flat[0].size
    rows = -(-n // C_)
    padded = [None if a is None else np.r_[a, np.full(rows * C_ - n, 0.5, a.dtype)].reshape(rows, C_) for a in flat]
    return [None if r is None else np.asarray(r).ravel()[:n] for r in fn(*padded)]


def threshold_limits(C_):
    lo = np.array([0.25, -np.inf, 0.0, 0.1, -np.inf] * 7)[:C_]
    hi = np.array([0.75, 0.5, np.inf, np.inf, np.inf] * 7)[:C_]
    return lo, hi


def threshold_values(n, C_, seed):
    rng = np.random.default_rng(seed)
    v = rng.random(n)
    lo, hi = threshold_limits(C_)
    for k, val in enumerate((0.25, 0.75, 0.5, 0.1, np.nan, np.inf, -np.inf, -0.0, 0.0, np.nextafter(0.25, 0), np.nextafter(0.75, 1))):
        v[(rng.integers(0, n, max(1, n // 23)))] = val                      # every special meets every channel over the sizes
    return v, 0.01 + rng.random(n), lo, hi


def run_thresholds(device, n, C_, v, s, lo, hi, configs=None):
    streams = [("val", np.float64, n, v), ("std", np.float64, n, s) if s is not None else None]

    def call(lib, stream, p):
        return lib.hm_apply_thresholds(p["val"], p.get("std"), f64(lo), f64(hi), n, C_, stream)
    return sweep(device, streams, call, f"hm_apply_thresholds n={n} C={C_}", configs, inplace=("val", "std"))


def assert_thresholds(got, n, C_, v, s, lo, hi, what):
    rv, rs = by_channel([v, s], C_, lambda a, b: orc.apply_thresholds(a, b, list(lo), list(hi)))
    assert_bits(got["val"], rv, what + " val")
    clipped = np.isnan(rv) & ~np.isnan(v)
    keep_expected = ~((v < np.resize(lo, n)) | (v > np.resize(hi, n)))      # (the strict comparison, per element e: channel e % C)
    assert np.array_equal(~clipped | np.isnan(v), keep_expected | np.isnan(v))
    if s is not None:
        assert_bits(got["std"], rs, what + " std")
        assert np.isnan(got["std"][clipped]).all() and np.array_equal(got["std"][~clipped].view(np.uint64), s[~clipped].view(np.uint64))
    assert np.array_equal(got["val"][~clipped].view(np.uint64), v[~clipped].view(np.uint64))


def check_thresholds(device, C_, sizes=None):
    sizes = sorted(set(SMALL + [C_ * 171 + 1, C_ * 7 + C_ // 2 + 1])) if sizes is None else sizes
    for n in sizes:
        v, s, lo, hi = threshold_values(n, C_, 100 * C_ + n)
        for with_std in (True, False):
            got = run_thresholds(device, n, C_, v, s if with_std else None, lo, hi)
            assert_thresholds(got, n, C_, v, s if with_std else None, lo, hi, f"thresholds n={n} C={C_} std={with_std}")


def check_thresholds_too_wide(device):
    with backend(device) as (lib, stream):
        b = Buf(device, np.float64, 66, 0, np.full(66, 9.0))
        lim = f64([0.0] * 33)
        assert lib.hm_apply_thresholds(b.ptr, None, lim, lim, 66, 33, stream) == nat.HM_EUNSUPPORTED
        assert np.all(b.get("C = 33") == 9.0)


# ------------------------------------------------------------------------------------------------ A, F, G: linearize
LIN_SIZES = sorted(set(SMALL + [383, 384, 385, 767, 769]))


def lin_tables(C_, rows=256, seed=5):
    rng = np.random.default_rng(seed)
    icrf = np.sort(rng.random((rows, C_)), axis=0)
    return icrf, rng.random((rows, C_)) + 0.5


def oracle_linearize(flat, sd, icrf, diff, C_, per_channel):
    """orc.linearize on the flat stream (channel = index % C) -> (val, std or None, idx)."""
    with np.errstate(all="ignore"):
        if not per_channel:
            return orc.linearize(flat, sd, icrf[:, 0], None if sd is None else diff[:, 0])
        return by_channel([flat, sd], C_, lambda a, b: orc.linearize(a, b, icrf, None if b is None else diff))


def run_linearize(device, kind, n, C_, per_channel, inp, sd, icrf, diff, want_idx=True, bits=None, configs=None):
    """kind: 'u8', 'f64', 'u16'."""
    in_t = {"u8": np.uint8, "f64": np.float64, "u16": np.uint16}[kind]
    idx_t = np.uint16 if kind == "u16" else np.uint8
    tab = icrf if per_channel else np.ascontiguousarray(icrf[:, 0])
    dtab = diff if per_channel else np.ascontiguousarray(diff[:, 0])
    ls = C_ if per_channel else 1
    streams = [("in", in_t, n, inp), ("sd", np.float64, n, sd) if sd is not None else None, ("icrf", np.float64, tab.size, tab),
               ("diff", np.float64, dtab.size, dtab) if sd is not None else None, ("val", np.float64, n, None),
               ("std", np.float64, n, None) if sd is not None else None, ("idx", idx_t, n, None) if want_idx and kind != "u8" else None]

    def call(lib, stream, p):
        if kind == "u8":
            return lib.hm_linearize_u8(p["in"], p.get("sd"), p["icrf"], p.get("diff"), p["val"], p.get("std"), n, C_, ls, stream)
        if kind == "f64":
            return lib.hm_linearize_f64(p["in"], p.get("sd"), p["icrf"], p.get("diff"), p["val"], p.get("std"), p.get("idx"), n, C_, ls, stream)
        return lib.hm_linearize_u16(p["in"], p.get("sd"), p["icrf"], p.get("diff"), p["val"], p.get("std"), p.get("idx"), n, C_, ls, bits, stream)
    if configs is None:
        configs = [None] + [i for i in (0, 1, 4, 5, 6) if streams[i] is not None]         # the tables are read element by element: not swept
    return sweep(device, streams, call, f"hm_linearize_{kind} n={n} C={C_} per_channel={per_channel} std={sd is not None}", configs)


def lin_f64_values(rng, n):
    v = rng.random(n)
    if n >= 3:
        m = max(1, n // 29)
        v[rng.integers(0, n, m)] = (rng.integers(0, 255, m) + 0.5) / 255.0   # ties: half to even
        v[rng.integers(0, n, m)] = rng.choice([-0.3, 1.7, 300.2, -0.0, 1.0, -1.0 / 255, 256.0 / 255], m)      # wrap modulo 256
    return v


def check_linearize(device, kind, sizes=LIN_SIZES):
    """hm_linearize_u8 / _f64: C = 3 per-channel tables and a single table; with and without std."""
    icrf, diff = lin_tables(3)
    for n in sizes:
        rng = np.random.default_rng(900 + n)
        inp = rng.integers(0, 256, n).astype(np.uint8) if kind == "u8" else lin_f64_values(rng, n)
        sd = stds(rng, n)
        for per_channel in (True, False):
            for with_std in (True, False):
                got = run_linearize(device, kind, n, 3, per_channel, inp, sd if with_std else None, icrf, diff)
                rv, rs, ri = oracle_linearize(inp, sd if with_std else None, icrf, diff, 3, per_channel)
                what = f"linearize_{kind} n={n} per_channel={per_channel} std={with_std}"
                assert_bits(got["val"], rv, what + " value")
                if with_std:
                    assert_bits(got["std"], rs, what + " std")
                if kind == "f64":
                    assert np.array_equal(got["idx"], ri), what + " index"


def check_linearize_channels(device, kind):
    """C = 1, 2, 4 per-channel tables (the general kernel's running channel counter), n not a multiple of C."""
    for C_ in (1, 2, 4):
        icrf, diff = lin_tables(C_, seed=C_)
        for n in (C_ * 200 + C_ // 2 + 1, 1025):
            rng = np.random.default_rng(n + C_)
            inp = rng.integers(0, 256, n).astype(np.uint8) if kind == "u8" else lin_f64_values(rng, n)
            sd = stds(rng, n)
            got = run_linearize(device, kind, n, C_, True, inp, sd, icrf, diff, configs=[None, 4])
            rv, rs, ri = oracle_linearize(inp, sd, icrf, diff, C_, True)
            assert_bits(got["val"], rv, f"linearize_{kind} C={C_} n={n}")
            assert_bits(got["std"], rs, f"linearize_{kind} C={C_} n={n} std")


UNDEFINED = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 2.0 ** 63 / 255 * 1.01, -2.0 ** 70, 4e16])
UNDEFINED_AT = {768: [0, 5, 130, 383, 384, 500, 766, 767], 383: [0, 1, 2, 127, 128, 255, 381, 382]}


def check_linearize_undefined(device):
    """F: index 0, the table's row 0, at the eight enumerated positions; every other element against the oracle."""
    icrf, diff = lin_tables(3)
    assert np.all((np.abs(UNDEFINED[3:] * 255.0) >= 2.0 ** 63))
    for n, at in UNDEFINED_AT.items():
        rng = np.random.default_rng(n)
        v, sd = lin_f64_values(rng, n), stds(rng, n)
        safe = v.copy()
        safe[at] = 0.0                                                       # index 0 by definition
        v[at] = UNDEFINED
        for per_channel in (True, False):
            got = run_linearize(device, "f64", n, 3, per_channel, v, sd, icrf, diff, configs=[None])
            rv, rs, ri = oracle_linearize(safe, sd, icrf, diff, 3, per_channel)
            assert np.array_equal(got["idx"][at], np.zeros(8, np.uint8)), (n, per_channel, got["idx"][at])
            assert np.array_equal(got["idx"], ri), f"linearize_f64 n={n}: index"
            assert_bits(got["val"], rv, f"linearize_f64 n={n} per_channel={per_channel}: row 0 at the undefined values")
            assert_bits(got["std"], rs, f"linearize_f64 n={n} per_channel={per_channel} std")


def check_linearize_u16(device, bits, sizes=SMALL):
    C_ = 3
    icrf, diff = lin_tables(C_, rows=1 << bits, seed=bits)
    mask = (1 << bits) - 1
    for n in sizes:
        rng = np.random.default_rng(bits * 10000 + n)
        dn = rng.integers(0, 65536, n).astype(np.uint16)                     # stray high bits above the bit depth
        dn[:3] = (mask, 0, 65535)[:min(n, 3)]
        sd = stds(rng, n)
        clean = (dn & mask).astype(np.int64)
        for per_channel in (True, False):
            for with_std in (True, False):
                for want_idx in (True, False):
                    got = run_linearize(device, "u16", n, C_, per_channel, dn, sd if with_std else None, icrf, diff, want_idx, bits,
                                        configs=None if want_idx and bits < 16 else [None, 0, 4])
                    rv, rs, ri = oracle_linearize(clean, sd if with_std else None, icrf, diff, C_, per_channel)
                    what = f"linearize_u16 bits={bits} n={n} per_channel={per_channel} std={with_std} idx={want_idx}"
                    assert_bits(got["val"], rv, what + " value")
                    if with_std:
                        assert_bits(got["std"], rs, what + " std")
                    if want_idx:
                        assert np.array_equal(got["idx"], clean), what + " index"


# ------------------------------------------------------------------------------------------------ the tests, on the host build
HOST = "cpu"


@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_binary_dense(op):
    check_binary_dense(HOST, op)


def test_difference():
    check_difference(HOST)


def test_interpolate():
    check_interpolate(HOST)


def test_unary():
    check_unary(HOST)


def test_log10_constant():
    check_log10_constant(HOST)


@pytest.mark.parametrize("p", EXPONENTS)
def test_pow_benign(p):
    check_pow_benign(HOST, p)


@pytest.mark.parametrize("p_index,p", list(enumerate(EXPONENTS + ODD_EXPONENTS)))
def test_pow_specials(p_index, p):
    check_pow_specials(HOST, p_index, p)


@pytest.mark.parametrize("p", [2.0, 0.5, -3.0, 2.5])
def test_pow_tail_specials(p):
    check_pow_tail_specials(HOST, p)


def test_pow_half_at_numpy():
    check_pow_half_at_numpy(HOST)


def test_binary_pow():
    check_binary_pow(HOST)


def test_weight_f64():
    check_weight_f64(HOST)


def test_weight_u8():
    check_weight_u8(HOST)


def test_u8_to_unit():
    check_u8_to_unit(HOST)


def test_take():
    check_take(HOST)


@pytest.mark.parametrize("op", [0, 1, 2, 3, 4])
def test_bcast_binary(op):
    check_bcast(HOST, "binary", op)


@pytest.mark.parametrize("entry", ["difference", "interpolate"])
def test_bcast_pointwise(entry):
    check_bcast(HOST, entry)


def test_bad_geometry():
    check_bad_geometry(HOST)


@pytest.mark.parametrize("C_", THRESHOLD_CHANNELS)
def test_thresholds(C_):
    check_thresholds(HOST, C_)


def test_thresholds_too_wide():
    check_thresholds_too_wide(HOST)


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_linearize(kind):
    check_linearize(HOST, kind)


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_linearize_channels(kind):
    check_linearize_channels(HOST, kind)


def test_linearize_undefined():
    check_linearize_undefined(HOST)


@pytest.mark.parametrize("bits", [9, 12, 16])
def test_linearize_u16(bits):
    check_linearize_u16(HOST, bits)


def test_reference_is_the_oracle():
    """The longdouble references written here against oracle.hdr_oracle's float64 evaluation at 1e-13, on benign values."""
    rng = np.random.default_rng(1)
    n = 400
    x, s = 0.05 + rng.random(n), 0.01 + 0.05 * rng.random(n)
    for p in (2.0, 0.5, 1.0, -3.0, 7.0, 2.5, -0.75):
        rv, rs = pow_reference(x, s, p)
        ov, os_ = orc.op_pow(x, s, np.array([p]), None)
        np.testing.assert_allclose(rv.astype(np.float64), ov, rtol=1e-13)
        np.testing.assert_allclose(rs.astype(np.float64), os_, rtol=1e-13)
    x2, s2 = 6 * rng.random(n) - 3, stds(rng, n)
    rv, rs = binary_pow_reference(x, s, x2, s2)
    ov, os_ = orc.op_pow(x, s, x2, s2)
    np.testing.assert_allclose(rv.astype(np.float64), ov, rtol=1e-13)
    np.testing.assert_allclose(rs.astype(np.float64), os_, rtol=1e-13)
    lx, ls = log_inputs(n, 2)
    for base10, fn in ((False, orc.op_log_e), (True, orc.op_log_10)):
        rv, rs = log_reference(lx, ls, base10)
        ov, os_ = fn(lx, ls)
        np.testing.assert_allclose(rv.astype(np.float64), ov, rtol=1e-13)
        np.testing.assert_allclose(rs.astype(np.float64), os_, rtol=1e-13)
    v = -1.5 + 4.0 * rng.random(n)
    rw, rdw = weight_reference(v)
    ow, odw = orc.gaussian_weight(v)
    np.testing.assert_allclose(rw.astype(np.float64), ow, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(rdw.astype(np.float64), odw, rtol=1e-13, atol=1e-300)
