"""The ICRF-calibration energy function (hm_linearity_energy) and the differential-evolution generation step (hm_de_generation,
hm_de_generation_batch) at the limits of their ABI, on the HOST build and on the NumPy oracle, against an extended-precision reference
written here from the formulas in the header of csrc/hm_energy.hip and in include/hdrmerge.h - not from oracle/ and not from the kernels.
The checks are functions of a device name: tests/test_gpu_energy_limits.py runs the same ones on the MI355X.

The reference (energy_reference)
    ratio = t_i / t_j, scaled = v_j ratio and d = v_i - scaled are float64: every implementation performs exactly these three IEEE
    operations, and d cancels, so any other rounding of them would be another function. Everything after them - d / scaled, sigma, the
    weight, every sum, the mean over the pairs - runs in np.longdouble (64-bit significand, asserted below). Two float64 facts are part
    of the function and are kept: a sigma^2 beyond float64's range is +inf in every implementation, so its weight is 0 and the sample
    is INCLUDED with zero weight; sigma == 0, a NaN sigma and a non-finite |d| exclude the sample.

The bound (pair_bound, energy_bound), u = 2^-53, first order in u
    Every summed term is >= 0, so a sum formed in ANY order with at most D additions on the path of a term is within D u (relative) of
    the exact sum of the terms as computed, and terms that carry T roundings each move it by at most T u more:
        |num - NUM| <= (T + D) u NUM,  |den - DEN| <= (T + D) u DEN,  result = num / den (one more rounding)
        => |result - RESULT| <= (2 (T + D) + 1) u RESULT.
    T, the roundings of a term after d, is counted on the pixel-major kernel, the worst case (1 / v_j by a 1.00 ulp = 2 u reciprocal,
    1 / sigma by a 1.25 ulp = 2.5 u reciprocal square root, every product u):
        unweighted absolute   |d| is exact                                                                          T = 0
        unweighted relative   inv_s = rcp(v_j) (1 / ratio): 2 + 1 + 1 = 4;  a = d inv_s: 5                        T = 5
        weighted absolute     w2 = ratio s_j: 1;  w2^2: 3;  s_i^2: 1;  q = s_i^2 + w2^2: 4;  w = rsq(q): 2 + 2.5 = 4.5;
                              a w: 5.5                                                                              T = 6
        weighted relative     a: 5;  u' = s_i inv_s: 5;  w2 = ((v_i s_j) inv_s) rcp(v_j): 1 + (4 + 1) + (2 + 1) = 9;
                              q = u'^2 + w2^2: max(11, 19) + 1 = 20;  w = rsq(q): 10 + 2.5 = 12.5;  a w: 18.5             T = 19
    (the pair-major kernel, the host build and the oracle use IEEE quotients and square roots: 9 at most in the last line). Rounding T
    up to an integer covers the second-order terms. D, the summation depth, is the implementation's documented structure:
        HIP kernels   ceil(P / (256 chunks)) additions per lane, 6 shuffle levels, 3 additions over the four waves, `chunks` additions
                      in k_energy_final;  chunks = hm_linearity_energy_workspace_bytes(P, N, B) / (16 B pairs), i.e. from the ABI
        host build    running sums in blocks of 1024 pixels: min(P, 1024) + ceil(P / 1024)
        NumPy oracle  pairwise summation: blocks of at most 128 terms in 8 accumulators (15 additions), 3 levels to combine them,
                      up to 7 leftover terms, one level per halving above 128: 25 + ceil(log2(n / 128)) (n additions below 8 terms)
    The energy is the mean of the non-NaN pair results, themselves >= 0 and each within its bound: the largest pair bound, plus
    (ceil(pairs / 64) + 6 + 1) u for k_energy_final's lane-strided sum, shuffle tree and division (host build: pairs + 1; oracle: its
    pairwise depth + 1). The reference's own error, about 40 x 2^-64 = 0.02 u, is inside the rounding of T. No margin is added.
    NaN and +inf patterns must be equal exactly. Every check prints the largest observed error in units of its bound."""
import functools
import math

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import icrf_calibration as ic
from oracle import hdr_oracle as orc

import test_de_batch_host as deb
import test_de_host as de

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the energy reference needs an extended-precision np.longdouble (x87: 64-bit significand)"
U = 2.0 ** -53
DBL_MAX = LD(np.finfo(np.float64).max)
T_ROUNDINGS = {(False, False): 0, (False, True): 5, (True, False): 6, (True, True): 19}     # (with_std, use_relative)
MODES = [(False, True), (False, False), (True, True), (True, False)]
WORST = {}                                                                                   # family -> largest error / bound seen


@pytest.fixture(scope="module", autouse=True)
def report_observed_maxima():
    """After the module's tests: the largest error of each family in units of its bound (DESIGN.md section 5 quotes them)."""
    yield
    print("\nobserved maxima, in units of the bound:", {k: round(v, 4) for k, v in sorted(WORST.items())})


# ------------------------------------------------------------------------------------------------ 1: the reference
def energy_reference(icrfs, dn, sd, t, lower, upper, relative):
    """icrfs (B, 256) float64 LUT values, dn (P, N) uint8, sd (P, N) float64 or None, t (N) float64 -> (pairs (B, N(N-1)/2), energies (B))
    in np.longdouble: NaN for a pair without a contributing sample, +inf for an energy without a non-NaN pair."""
    icrfs, t = np.atleast_2d(np.asarray(icrfs, np.float64)), np.asarray(t, np.float64)
    B, N = icrfs.shape[0], dn.shape[1]
    v = icrfs[:, dn.astype(np.intp)]                                         # (B, P, N)
    lo, hi = icrfs[:, lower, None, None], icrfs[:, upper, None, None]
    v = np.where((v < lo) | (v > hi), np.nan, v)
    out = []
    with np.errstate(all="ignore"):
        for i in range(N):
            for j in range(i + 1, N):
                ratio = t[i] / t[j]                                          # float64, one IEEE division
                vi, vj = v[:, :, i], v[:, :, j]
                scaled = vj * ratio                                          # float64, one IEEE product
                d = (vi - scaled).astype(LD)                                 # float64, one IEEE difference; extended from here on
                a = np.abs(d / scaled.astype(LD)) if relative else np.abs(d)
                if sd is None:
                    keep = ~np.isnan(a)
                    w = keep.astype(LD)
                else:
                    si, sj = sd[None, :, i].astype(LD), sd[None, :, j].astype(LD)
                    if relative:
                        q = (si / scaled.astype(LD)) ** 2 + ((vi.astype(LD) * sj) / (LD(ratio) * vj.astype(LD) ** 2)) ** 2
                    else:
                        q = si ** 2 + (LD(ratio) * sj) ** 2
                    sigma = np.sqrt(q)
                    keep = np.isfinite(a) & (sigma != 0) & ~np.isnan(sigma)
                    w = np.where(q > DBL_MAX, LD(0), LD(1) / sigma)          # float64's sigma is +inf there: weight 0, sample included
                num = np.where(keep, a * w, LD(0)).sum(axis=1)
                den = np.where(keep, w, LD(0)).sum(axis=1)
                out.append(np.where(den != 0, num / den, LD(np.nan)))
        pairs = np.stack(out, axis=1)
        fin = ~np.isnan(pairs)
        e = np.where(fin, pairs, LD(0)).sum(axis=1) / fin.sum(axis=1)
    return pairs, np.where(np.isnan(e), LD(np.inf), e)


def test_reference_matches_the_golden_energy_vectors(golden):
    """The reference against the vectors the reference PROJECT produced (tests/golden/energy.npz), at float64's own accuracy: the
    project sums in float64 (pairwise), so 1e-13."""
    g = golden("energy")
    dn, sd, t, lo, up = g["dn"].reshape(-1, 5), g["sd"].reshape(-1, 5), g["exposures"], int(g["lower"]), int(g["upper"])
    ok = np.isfinite(g["energy_plain"])
    assert 0 < ok.sum() < len(ok)
    for s, ekey, pkey in ((None, "energy_plain", "pairs_plain"), (sd, "energy_std", "pairs_std")):
        pairs, e = energy_reference(g["icrfs"][ok], dn, s, t, lo, up, True)
        np.testing.assert_allclose(e.astype(np.float64), g[ekey][ok], rtol=1e-13)
        np.testing.assert_allclose(pairs.astype(np.float64), g[pkey][ok], rtol=1e-13, equal_nan=True)
    for s, key in ((None, "abs_plain"), (sd, "abs_std")):
        pairs, _ = energy_reference(g["icrfs"][:1], dn, s, t, lo, up, False)
        np.testing.assert_allclose(pairs[0].astype(np.float64), g[key], rtol=1e-13, equal_nan=True)


def test_reference_specials():
    """Empty pair -> NaN, empty energy -> +inf, an overflowing sigma -> included with weight 0, v_j = 0 -> an infinite unweighted pair."""
    icrf = np.linspace(0, 1, 256)[None]
    t = np.array([1.0, 2.0])
    dn = np.array([[100, 200], [50, 120]], np.uint8)
    p, e = energy_reference(icrf, dn, None, t, 200, 100, True)
    assert np.isnan(p).all() and np.isinf(e).all()
    huge = np.array([[1e200, 1.0], [1.0, 1.0]])
    p1, _ = energy_reference(icrf, dn, huge, t, 5, 250, True)
    p2, _ = energy_reference(icrf, dn[1:], huge[1:], t, 5, 250, True)
    assert p1[0, 0] == p2[0, 0] and np.isfinite(p1[0, 0])                  # the 1e200 sample weighs nothing
    p3, _ = energy_reference(icrf, dn[:1], huge[:1], t, 5, 250, True)
    assert np.isnan(p3[0, 0])                                              # alone it leaves sum(w) == 0
    p4, e4 = energy_reference(icrf, np.array([[9, 0]], np.uint8), None, t, 0, 255, True)
    assert np.isposinf(p4[0, 0]) and np.isposinf(e4[0])


# ------------------------------------------------------------------------------------------------ 2: the bound
def chunks_of(P, N, B):
    """The pixel chunks of a HIP launch, from the ABI's workspace size: (B, pairs, chunks, 2) float64."""
    pairs = N * (N - 1) // 2
    ws = nat.hip_lib.hm_linearity_energy_workspace_bytes(P, N, B)
    assert ws > 0 and ws % (16 * B * pairs) == 0
    return ws // (16 * B * pairs)


def np_depth(n):
    return n if n < 8 else 25 + max(0, math.ceil(math.log2(n / 128)))


def depths(family, P, N, B):
    """-> (summation depth of a pair result, additions + division of the energy) of an implementation family."""
    pairs = N * (N - 1) // 2
    if family == "host":
        return min(P, 1024) + -(-P // 1024), pairs + 1
    if family == "oracle":
        return np_depth(P), np_depth(pairs) + 1
    c = chunks_of(P, N, B)
    return -(-P // (256 * c)) + 6 + 3 + c, -(-pairs // 64) + 6 + 1


def pair_bound(family, with_std, relative, P, N, B):
    return (2 * (T_ROUNDINGS[(with_std, relative)] + depths(family, P, N, B)[0]) + 1) * U


def energy_bound(family, with_std, relative, P, N, B):
    return pair_bound(family, with_std, relative, P, N, B) + depths(family, P, N, B)[1] * U


def test_bound_counts():
    assert chunks_of(37 * 31, 4, 3) == 2 and chunks_of(129 * 128, 3, 8) == 17 and chunks_of(257 * 257, 3, 8) == 64 and chunks_of(1, 3, 3) == 1
    assert depths("hip", 257 * 257, 3, 8) == (5 + 6 + 3 + 64, 8) and depths("hip", 132, 32, 3) == (1 + 6 + 3 + 1, 8 + 6 + 1)
    assert depths("host", 66049, 3, 8) == (1024 + 65, 4) and depths("oracle", 66049, 3, 8) == (25 + 10, 4)
    assert pair_bound("hip", True, True, 132, 32, 3) == (2 * (19 + 11) + 1) * U < 1e-14


def assert_within(got, ref, bound, family, what):
    """got float64, ref longdouble, same shape: NaN / inf patterns equal, finite entries within `bound` (relative) of ref.
    -> the largest error in units of the bound (recorded per family)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, LD)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{what}: NaN pattern")
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref), err_msg=f"{what}: +inf pattern")
    assert not np.isneginf(got).any() and not np.isneginf(ref).any(), what
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    g, r = got[fin], ref[fin]
    assert np.all(g[r == 0] == 0), what                                     # (a relative bound: an exact zero stays one)
    nz = r != 0
    worst = float((np.abs(g[nz].astype(LD) - r[nz]) / (LD(bound) * np.abs(r[nz]))).max()) if nz.any() else 0.0
    WORST[family] = max(WORST.get(family, 0.0), worst)
    assert worst <= 1.0, f"{what}: {worst:.3f} x the bound of {bound / U:.0f} u ({family})"
    return worst


# ------------------------------------------------------------------------------------------------ 3: the cases
def gammas(B, lo=0.6, hi=2.4):
    return np.stack([np.linspace(0, 1, 256) ** g for g in np.linspace(lo, hi, B)])


def reject(B, rows=(1,)):
    valid = np.ones(B, bool)
    valid[list(rows)] = False
    return valid


def base_case(seed, X, Y, N, B, sort=True, dn_range=(0, 256), t=None):
    rng = np.random.default_rng(seed)
    dn = rng.integers(*dn_range, (X, Y, N)).astype(np.uint8)
    if sort:
        dn = np.sort(dn, axis=2)
    return dict(dn=dn, sd=0.004 * (1 + rng.random((X, Y, N))), t=1e-3 * 2.0 ** np.arange(N) if t is None else t, icrfs=gammas(B),
                valid=reject(B), lower=5, upper=250, modes=MODES, finite=None, rng=rng)


def case_limits_0_255():
    """icrf[0] == 0 inside the limits: v_j = 0 under v_i > 0 makes |d / scaled| = inf, under v_i = 0 NaN. The unweighted relative pair
    is then +inf and the energy +inf; the weighted pair and absolute mode drop or never form those samples."""
    c = base_case(31, 37, 31, 4, 3, sort=False)
    c["dn"][c["rng"].random(c["dn"].shape) < 0.04] = 0
    c["dn"][::6, ::5] = 0
    c.update(lower=0, upper=255, finite=lambda ws, rel: 0 if (rel and not ws) else 2 * 6)
    assert np.all(c["icrfs"][:, 0] == 0)
    for i in range(4):
        for j in range(i + 1, 4):
            assert np.any((c["dn"][..., j] == 0) & (c["dn"][..., i] > 0)) and np.any((c["dn"][..., j] == 0) & (c["dn"][..., i] == 0))
    return c


def case_limits_equal():
    c = base_case(32, 37, 31, 3, 3)
    c["dn"][::9, ::7] = 128                                   # only samples AT the limit survive: pixels that read 128 in every frame
    c.update(lower=128, upper=128)
    return c


def case_limits_reversed():
    c = base_case(33, 37, 31, 3, 3)
    c.update(lower=200, upper=100, finite=lambda ws, rel: 0)
    return c


def case_nonmonotone():
    """Candidates that are not monotone, passed with valid=None: the limits apply to VALUES (v < icrf[lower] or v > icrf[upper]), not
    to DNs - the two readings differ in more than 5 % of the samples of every candidate (asserted)."""
    c = base_case(34, 37, 31, 4, 3)
    x = np.linspace(0, 1, 256)
    icrfs = np.stack([x + amp * np.sin(4 * np.pi * x) for amp in (0.15, 0.2, 0.25)])
    icrfs[:, 0], icrfs[:, 255] = 0.0, 1.0
    assert np.all(np.diff(icrfs, axis=1).min(axis=1) < 0)
    c.update(icrfs=icrfs, valid=None, lower=40, upper=215)
    for row in icrfs:
        v = row[c["dn"]]
        by_value, by_dn = (v < row[40]) | (v > row[215]), (c["dn"] < 40) | (c["dn"] > 215)
        assert np.mean(by_value != by_dn) >= 0.05
    return c


def case_std_specials():
    c = base_case(35, 37, 31, 4, 3)
    r = c["rng"].random(c["sd"].shape)
    c["sd"][r < 0.05] = 0.0
    c["sd"][(r >= 0.05) & (r < 0.10)] = np.inf
    c["sd"][(r >= 0.10) & (r < 0.15)] = np.nan
    assert all(abs(np.mean(m) - 0.05) < 0.01 for m in (c["sd"] == 0, np.isinf(c["sd"]), np.isnan(c["sd"])))
    c.update(modes=[(True, True), (True, False)], finite=lambda ws, rel: ("min", 1))
    return c


def case_std_huge():
    """sigma overflows where std is 1e200: the weight is 0 and the sample counts as included."""
    c = base_case(36, 37, 31, 4, 3)
    c["sd"][c["rng"].random(c["sd"].shape) < 0.01] = 1e200
    assert 3 <= (c["sd"] == 1e200).sum() <= 200
    c.update(modes=[(True, True), (True, False)], finite=lambda ws, rel: ("min", 1))
    return c


def case_std_huge_only():
    """Every sample of frame 0 has an overflowing sigma: its three pairs have sum(w) == 0 and are NaN, the other three are finite."""
    c = case_std_huge()
    c["sd"][..., 0] = 1e200
    c.update(finite=lambda ws, rel: 2 * 3)
    return c


def case_many_candidates():
    c = base_case(37, 8, 8, 3, 1024, dn_range=(6, 250))
    c.update(valid=np.arange(1024) % 2 == 0, icrfs=gammas(1024, 0.5, 2.5))
    return c


def case_n32():
    c = base_case(38, 12, 11, 32, 3, t=1e-3 * 1.25 ** np.arange(32))
    c.update(finite=lambda ws, rel: ("min", 2 * 400))
    return c


CASES = {f"frames_{n}": functools.partial(base_case, 10 + n, 37, 31, n, 3) for n in range(2, 9)}
CASES.update({f"pixels_{p}": functools.partial(base_case, 20 + k, p, 1, 3, 3, dn_range=(6, 250))
              for k, p in enumerate((1, 2, 255, 257, 1024, 1025))})
CASES.update({
    "pair_major_4_frames": functools.partial(base_case, 40, 129, 128, 4, 3),          # P > 16 384 and B < 8: the pair-major kernel
    "pair_major_8_frames": functools.partial(base_case, 41, 129, 128, 8, 3),
    "pair_major_9_frames": functools.partial(base_case, 42, 12, 11, 9, 3),
    "pair_major_32_frames": case_n32,
    "pixel_major_17_chunks": functools.partial(base_case, 43, 129, 128, 3, 8),
    "pixel_major_64_chunks": functools.partial(base_case, 44, 257, 257, 3, 8),        # 66 049 pixels: the cap of 64 chunks binds
    "limits_0_255": case_limits_0_255, "limits_equal": case_limits_equal, "limits_reversed": case_limits_reversed,
    "nonmonotone": case_nonmonotone, "std_specials": case_std_specials, "std_huge": case_std_huge, "std_huge_only": case_std_huge_only,
    "many_candidates": case_many_candidates,
})
GEOMETRY = {"pair_major_4_frames": False, "pair_major_8_frames": False, "pair_major_9_frames": False, "pair_major_32_frames": False}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c.pop("rng")
    c["dn"].setflags(write=False)
    c["sd"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference_of(name, with_std, relative):
    """The reference of a case, computed once per session, shared by the host, oracle and device checks, never modified; with the
    assertion on how many finite pairs it holds."""
    c = case(name)
    N = c["dn"].shape[2]
    rows = np.arange(len(c["icrfs"])) if c["valid"] is None else np.nonzero(c["valid"])[0]
    pairs, e = energy_reference(c["icrfs"][rows], c["dn"].reshape(-1, N), c["sd"].reshape(-1, N) if with_std else None, c["t"],
                                c["lower"], c["upper"], relative)
    n_finite, n_pairs = int(np.isfinite(pairs).sum()), N * (N - 1) // 2
    want = len(rows) * n_pairs if c["finite"] is None else c["finite"](with_std, relative)
    if isinstance(want, tuple):
        assert n_finite >= want[1], (name, with_std, relative, n_finite, want)
    else:
        assert n_finite == want, (name, with_std, relative, n_finite, want)
    all_pairs = np.full((len(c["icrfs"]), n_pairs), LD(np.nan))
    all_e = np.full(len(c["icrfs"]), LD(np.inf))
    all_pairs[rows], all_e[rows] = pairs, e
    for a in (all_pairs, all_e):
        a.setflags(write=False)
    return all_pairs, all_e, n_finite


def family_of(device, name):
    if not str(device).startswith("cuda"):
        return "host"
    return "pixel-major" if GEOMETRY.get(name, True) else "pair-major"


def run_energy(device, c, with_std, relative, rows=None, valid="case"):
    dn = torch.tensor(c["dn"], device=device)                                 # (copies: the case's arrays are read-only)
    sd = torch.tensor(c["sd"], device=device) if with_std else None
    icrfs = c["icrfs"] if rows is None else c["icrfs"][rows]
    valid = c["valid"] if isinstance(valid, str) else valid
    e, pairs = ic._engine_for(dn).linearity_energy(dn, sd, c["t"], icrfs, c["lower"], c["upper"], valid, relative, return_pairs=True)
    return pairs.cpu().numpy(), e.cpu().numpy()


def check_energy_case(device, name):
    c = case(name)
    X, Y, N = c["dn"].shape
    P, B = X * Y, len(c["icrfs"])
    family = family_of(device, name)
    if family != "host":
        assert (N <= 8 and (B >= 8 or P <= 16384)) == (family == "pixel-major")          # the launcher's documented rule
    for with_std, relative in c["modes"]:
        ref_pairs, ref_e, n_finite = reference_of(name, with_std, relative)
        pairs, e = run_energy(device, c, with_std, relative)
        what = f"{name} std={with_std} relative={relative}"
        if c["valid"] is not None:
            assert np.isnan(pairs[~c["valid"]]).all() and np.isposinf(e[~c["valid"]]).all(), what
        wp = assert_within(pairs, ref_pairs, pair_bound(family, with_std, relative, P, N, B), family, what + " pairs")
        we = assert_within(e, ref_e, energy_bound(family, with_std, relative, P, N, B), family, what + " energy")
        print(f"{what} [{family}]: {n_finite} finite reference pairs, worst pair {wp:.3f}, worst energy {we:.3f} of the bound "
              f"({pair_bound(family, with_std, relative, P, N, B) / U:.0f} u)")


def check_oracle_case(name):
    """The NumPy oracle (one candidate per call) under the same bound, with its own summation depth."""
    c = case(name)
    X, Y, N = c["dn"].shape
    rows = (np.arange(len(c["icrfs"])) if c["valid"] is None else np.nonzero(c["valid"])[0])[:4]
    for with_std, relative in c["modes"]:
        ref_pairs, ref_e, _ = reference_of(name, with_std, relative)
        for b in rows:
            row = c["icrfs"][b]
            got = orc.analyze_linearity_pairs(row[c["dn"]], c["sd"] if with_std else None, row[c["lower"]], row[c["upper"]], relative, c["t"])
            what = f"oracle {name} std={with_std} relative={relative} row {b}"
            assert_within(got, ref_pairs[b], pair_bound("oracle", with_std, relative, X * Y, N, 1), "oracle", what)
            if relative and c["valid"] is not None:                                      # (energy_function applies its own verdict)
                assert_within(orc.energy_function(row, c["dn"], c["sd"] if with_std else None, c["lower"], c["upper"], c["t"]),
                              ref_e[b], energy_bound("oracle", with_std, relative, X * Y, N, 1), "oracle", what + " energy")


def check_both_geometries(device):
    """One stack, one reference: eight candidates take the pixel-major kernel, a lone candidate on the same 16 512 pixels the
    pair-major one. Both lie within their bounds."""
    name = "pixel_major_17_chunks"
    c = case(name)
    X, Y, N = c["dn"].shape
    cuda = str(device).startswith("cuda")
    for with_std, relative in MODES:
        ref_pairs, ref_e, _ = reference_of(name, with_std, relative)
        pairs8, e8 = run_energy(device, c, with_std, relative)
        pairs1, e1 = run_energy(device, c, with_std, relative, rows=[0], valid=None)
        for got_p, got_e, rows, B, family in ((pairs8, e8, slice(None), 8, "pixel-major"), (pairs1, e1, slice(0, 1), 1, "pair-major")):
            family = family if cuda else "host"
            assert_within(got_p, ref_pairs[rows], pair_bound(family, with_std, relative, X * Y, N, B), family, f"{family} B={B} pairs")
            assert_within(got_e, ref_e[rows], energy_bound(family, with_std, relative, X * Y, N, B), family, f"{family} B={B} energy")
        print(f"std={with_std} relative={relative}: pixel-major and pair-major pair results of candidate 0 "
              f"{'equal' if np.array_equal(pairs8[0], pairs1[0]) else 'differ'} bit for bit")


@pytest.mark.parametrize("name", list(CASES))
def test_energy_case_host(name):
    check_energy_case("cpu", name)


@pytest.mark.parametrize("name", list(CASES))
def test_energy_case_oracle(name):
    check_oracle_case(name)


def test_both_geometries_host():
    check_both_geometries("cpu")


# ------------------------------------------------------------------------------------------------ 4: the generation step at the limits
DE_SHAPE = (24, 24, 5)
DE_CASES = [(4, 1), (5, 3), (7, 2), (45, 3), (75, 5), (257, 3), (1000, 3), (1024, 32), (4, 32)]
# (seed of the initial population, members near the optimum per 8, their spread) per (S, P): chosen on the host build so that in every
# checked generation at least a quarter of the trial rows are valid and at least one is not, and no input sits on a threshold
DE_SETUP = {(4, 1): (402, 5, 0.1), (5, 3): (505, 4, 0.02)}                 # every other case: (100 S + P, 6, 0.1)


def make_problem(device, P, shape=DE_SHAPE):
    """test_de_host.make_problem for up to HM_DE_MAX_PARAMS components: the same sine basis, the true parameters padded with zeros."""
    X, Y, N = shape
    rng = np.random.default_rng(21)
    t = 1e-3 * 2.0 ** np.arange(N)
    xs = np.linspace(0, 1, 256)
    pca = np.stack([np.sin(np.pi * (m + 1) * xs) / (m + 1) for m in range(P)], axis=1) * 0.1
    mean_icrf = xs ** 2.0
    true_params = np.zeros(P)
    true_params[: min(P, 5)] = [0.6, -0.3, 0.2, 0.1, -0.1][:P]
    true_icrf, ok = ic.candidate_icrfs(true_params, mean_icrf, pca)
    assert ok[0]
    lin = np.clip((rng.random((X, Y)) * 2.5 / t[-1])[..., None] * t, 0, 1)
    dn = np.clip(np.around(np.interp(lin, true_icrf[0], xs) * 255), 0, 255).astype(np.uint8)
    return dict(stack=torch.as_tensor(dn, device=device), dn=dn, t=t, pca=pca, mean=mean_icrf, true=true_params, P=P, device=device)


def initial_population(pr, S, P):
    seed, near8, spread = DE_SETUP.get((S, P), (100 * S + P, 6, 0.1))
    rng = np.random.default_rng(seed)
    pop = rng.random((S, P))
    n_near = max(1, min(S - 1, (S * near8) // 8))
    pop[:n_near] = 0.5 * (pr["true"] + 1) + spread * (rng.random((n_near, P)) - 0.5)
    return pop


def check_generation_at_limits(device, S, P, generations=(1, 2, 123456), strict=True):
    """check_one_generation of test_de_host.py at the ABI's limits of S and P, with the trial energies held to the extended-precision
    reference under the derived bound instead of to the energy entry point. -> (valid rows, invalid rows) per generation."""
    pr = make_problem(device, P)
    family = "pixel-major" if str(device).startswith("cuda") else "host"
    n_pix, N = pr["dn"].shape[0] * pr["dn"].shape[1], pr["dn"].shape[2]
    seed = 1234 + S
    plan = de.make_plan(pr, initial_population(pr, S, P), seed=seed)
    plan.launch()
    st = plan.read_status()
    assert st["generation"] == 0 and st["evaluations"] == S and st["stop"] == 0
    assert st["best_index"] == int(np.argmin(de.host(plan.energies)))
    counts = []
    for g in generations:
        de.poke(plan, nat.HM_DE_GENERATION, g)
        de.poke(plan, nat.HM_DE_STOP, 0)
        pop, E, best = de.host(plan.population), de.host(plan.energies), plan.read_status()["best_index"]
        assert best == int(np.argmin(E))
        ref = de.np_trial(pop, best, g, seed)
        m = ref["mutant"][ref["taken"]]
        assert np.all(np.minimum(np.abs(m), np.abs(m - 1)) > 1e-12)                      # no mutant component at the edge of [0, 1]
        plan.launch()
        trial = de.host(plan.trial)
        keep = ~ref["taken"]
        np.testing.assert_array_equal(trial[keep], pop[keep])                            # crossover mask and fill point: exact
        assert ref["taken"].any(axis=1).all()
        np.testing.assert_array_equal(trial[ref["replaced"]], ref["redraw"][ref["replaced"]])   # out-of-range replacements: exact draws
        np.testing.assert_allclose(trial, ref["trial"], rtol=0, atol=1e-14)
        icrfs, valid = ic.candidate_icrfs(-1.0 + trial * 2.0, pr["mean"], pr["pca"])
        assert np.all(icrfs[:, 255] == 1.0) and np.all(icrfs[:, 0] == 0.0)
        inner = icrfs[:, 1:255]
        assert np.abs(inner).min() > 1e-9 and np.abs(inner - 1).min() > 1e-9             # no entry within 1e-9 of the range limits
        assert np.abs(np.diff(icrfs, axis=1)).min() > 1e-9                               # no step within 1e-9 of zero
        counts.append((int(valid.sum()), int((~valid).sum())))
        if strict:
            assert 4 * valid.sum() >= S and (~valid).any(), (S, P, g, counts)
        dev_icrf = de.host(plan.icrf)
        np.testing.assert_allclose(dev_icrf, icrfs, rtol=0, atol=1e-13)
        np.testing.assert_array_equal(de.host(plan.valid).astype(bool), valid)
        Et = de.host(plan.trial_energies)
        assert np.all(np.isposinf(Et[~valid]))
        _, e_ref = energy_reference(dev_icrf[valid], pr["dn"].reshape(-1, N), None, pr["t"], 5, 250, True)
        assert np.isfinite(e_ref).all()
        worst = assert_within(Et[valid], e_ref, energy_bound(family, False, True, n_pix, N, S), family, f"DE S={S} P={P} g={g} trial energies")
        pop2, E2, best2, mean, sd, stop, _ = de.np_select(pop, E, trial, Et, g)
        st = plan.read_status()
        np.testing.assert_array_equal(de.host(plan.population), pop2)
        np.testing.assert_array_equal(de.host(plan.energies), E2)
        assert st["best_index"] == best2 and st["best_energy"] == E2[best2] and st["stop"] == stop and st["generation"] == g
        np.testing.assert_allclose(st["mean"], mean, rtol=1e-12)
        np.testing.assert_allclose(st["std"], sd, rtol=1e-12, equal_nan=True)
        print(f"S={S} P={P} g={g}: {counts[-1][0]} valid / {counts[-1][1]} invalid rows, replaced={int(ref['replaced'].sum())}, "
              f"worst energy {worst:.3f} of the bound")
    return counts


@pytest.mark.parametrize("S,P", DE_CASES)
def test_generation_at_limits_host(S, P):
    check_generation_at_limits("cpu", S, P)


def check_ties_above_256(device):
    """Members 300..599 of 600 are one point, better than the others: the winner is the first of them, through the padded tree's
    levels above one workgroup's width."""
    pr = make_problem(device, 3)
    rng = np.random.default_rng(8)
    pop = np.tile(0.5 * (pr["true"] + 1), (600, 1))
    pop[:300] += 0.1 + 0.1 * rng.random((300, 3))
    plan = de.make_plan(pr, pop)
    plan.launch()
    E = de.host(plan.energies)
    assert np.all(E[300:] == E[300]) and np.isfinite(E[300]) and E[300] < E[:300].min() and np.isfinite(E[:300]).sum() >= 75
    st = plan.read_status()
    assert st["best_index"] == 300 and st["best_energy"] == E[300]


def test_ties_above_256_host():
    check_ties_above_256("cpu")


def check_batch_of_64(device):
    """K = HM_DE_MAX_PROBLEMS problems of the smallest population on 64 distinct stacks, distinct seeds: every problem evolves as alone."""
    b = deb.make_batch(device, 64, (8, 8, 4), 4, 3, seeds=range(500, 564))
    batch, _ = deb.step_both(b, 3)
    E = de.host(batch.energies)
    assert len({E[k].tobytes() for k in range(64)}) == 64 and np.isfinite(E).any()


def check_batch_of_3_with_45(device):
    """K = 3, S = 45 (a padded selection tree in every problem): against single plans after every generation, and generation 1
    against the NumPy restatement problem by problem."""
    seeds = (21, 22, 23)
    b = deb.make_batch(device, 3, (24, 24, 5), 45, 3, seeds=seeds)
    batch, singles = deb.batch_plan(b), deb.single_plans(b)
    for g in range(4):
        if g == 1:
            before = [(de.host(batch.population[k]), de.host(batch.energies[k]), batch.read_status()[k]["best_index"]) for k in range(3)]
        batch.launch()
        for p in singles:
            p.launch()
        deb.assert_batch_equals_singles(batch, singles)
        if g == 1:
            for k, (pop, E, best) in enumerate(before):
                assert best == int(np.argmin(E))
                ref = de.np_trial(pop, best, 1, seeds[k])
                trial, Et = de.host(batch.trial[k]), de.host(batch.trial_energies[k])
                np.testing.assert_array_equal(trial[~ref["taken"]], pop[~ref["taken"]])
                np.testing.assert_array_equal(trial[ref["replaced"]], ref["redraw"][ref["replaced"]])
                np.testing.assert_allclose(trial, ref["trial"], rtol=0, atol=1e-14)
                pop2, E2, best2, mean, sd, stop, _ = de.np_select(pop, E, trial, Et, 1, tol=0.0)
                st = batch.read_status()[k]
                np.testing.assert_array_equal(de.host(batch.population[k]), pop2)
                np.testing.assert_array_equal(de.host(batch.energies[k]), E2)
                assert st["best_index"] == best2 and st["best_energy"] == E2[best2] and st["stop"] == stop and st["generation"] == 1
                np.testing.assert_allclose(st["mean"], mean, rtol=1e-12)
                np.testing.assert_allclose(st["std"], sd, rtol=1e-12, equal_nan=True)


def test_batch_of_64_host():
    check_batch_of_64("cpu")


def test_batch_of_3_with_45_host():
    check_batch_of_3_with_45("cpu")
