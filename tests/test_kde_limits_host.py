"""The kernel density estimate (csrc/hm_kde.hip: k_kde_moments1 / k_kde_moments2 / k_kde_finish, k_kde_eval, k_kde_sum) at the limits
of its ABI, on the HOST build (csrc_host/hm_host.cpp), against references in extended precision written here - no SciPy: it whitens in
float64 too and cannot arbitrate at this precision. The checks are functions of a device name; tests/test_gpu_kde_limits.py runs the same
ones on the MI355X. hm_kde_moments and hm_kde_evaluate are called through the raw C ABI with h, scale and the grid given by the test;
out, moments and the workspace lie between 64-byte canaries.

Reference of the estimate (evaluate_reference)
    estimate[j] = scale * sum_i w_i exp(-((x_i - y_j) / h)^2 / 2) over the counted elements (finite x; with std, std != 0), w_i = 1 / std_i
    or 1, every operation in np.longdouble (64-bit significand, e = 2^-64). test_reference_against_mpmath checks that reference against
    mpmath at 40 digits on every case of at most 4096 elements (a subset of the grid points where elements x points would exceed 12 000).

Bound of the estimate (evaluate_bound) - from the reference alone, u = 2^-53
    The kernel forms, in float64, U = fl(x / h), V = fl(y / h), D = fl(U - V), A = fl(fl(D D) 0.5), E = exp(-A), T = fl(w E),
    w = fl(1 / std). With |U - x/h| <= u |x/h| etc. and d = (x - y) / h:
        |D - d|     <= u (|x/h| + |y/h|) + u |d|                                 two quotients, one subtraction
        |A - d^2/2| <= |d| |D - d| + u d^2 / 2  = u (|d| (|x/h| + |y/h|) + 1.5 d^2)     the square's rounding; * 0.5 is exact
        exp(-A) = exp(-d^2/2) (1 + (A - d^2/2)) to first order, and the library's exp is good to 1 ulp = 2 u; fl(1 / std), the product
        w E and the final product with `scale` add u each:
        |T - t| / |t| <= u (|d| (|x/h| + |y/h|) + c1 d^2 + c2),     c1 = 1.5,  c2 = 2 + 1 + 1 + 1 = 5
    The sum: a chunk's tiles follow each other in one accumulator, slice s of k_kde_sum adds chunks s, s + 16, ... (ceil(chunks / 16)
    additions), the 16 slices are added in order (16), and the elements of a tile are added one after the other: log2(n) stands for
    that chain - a model of rounding errors of either sign, not its worst case, which would be the tile's 1023 - so
        sum:  (tiles in a chunk + ceil(chunks / 16) + 16 + log2 n) u sum_i |t_i|
    (host build: chunks of 4096 COUNTED elements, i.e. 4 tiles, added in order: 4 + ceil(counted / 4096) + log2 n).
    Results below 2^-1022 are subnormal, their spacing is 2^-1074 whatever their size: an underflowing exp, product or total adds at most
    (sum_i |w_i| + counted + 1) 2^-1074 max(scale, 1). The reference's own error - the same per-term expression with e for u - is added.
    The asserted bound is TWICE the sum of these (second-order terms). test_restatement_within_bound checks, without any kernel, that a
    float64 NumPy restatement of the device's operation sequence stays inside it for every input of this file.

Moments (moments_reference, moments_bound)
    count, min, max and the three flag counts are exact. sum w, sum w^2, sum w x and sum w (x - x_bar)^2 are summed exactly (math.fsum
    over the float64 halves of longdouble products, w = fl(1 / std) as kde_load defines it). A value passes D additions:
        HIP   a lane's chain of ceil(n / 131072), 6 shuffle steps, 3 additions over the 4 waves, k_kde_finish: a chain of 8 and 6
              shuffle steps: D = ceil(n / 131072) + 23          host  256 slices in order: D = ceil(n / 256) + 256
        |sum w - ref| <= D u sum|w|;  sum w^2, sum w x: (D + 1) u sum|.|;  x_bar = fl(sum w x / sum w): its two sums' errors and u |x_bar|;
        m2: (D + 4) u sum |w| (x - x_bar)^2 + 2 db sum |w| |x - x_bar| + db^2 sum|w|,  db = the bound of x_bar
    again twice that. Where the reference is not finite (a NaN or subnormal std) the pattern NaN / +inf / -inf must agree.

Every check records its largest error as a fraction of its bound; the module prints the maxima at its end (DESIGN.md 4.4.2 quotes them)."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the references need an extended-precision np.longdouble (x87: 64-bit significand)"
U = 2.0 ** -53
E_LD = LD(2.0) ** -64
C1, C2 = 1.5, 5.0
TILE, TARGET_CHUNKS, BLOCK_PTS, MOM_LANES, MOM_BYTES = 1024, 2048, 1024, 512 * 256, 512 * 16 * 8   # hm_kde.hip's constants
HOST_CHUNK, HOST_SLICES = 4096, 256                                                                 # hm_host.cpp's
TINY = LD(2.0) ** -1074
WORST = {}                                                                  # family -> largest error / bound seen


@pytest.fixture(scope="module", autouse=True)
def report_observed_maxima():
    """After the module's tests: the largest error of each case group in units of its bound."""
    yield
    print("\nobserved maxima, in units of the bound:", {k: round(v, 4) for k, v in sorted(WORST.items())})


# ------------------------------------------------------------------------------------------------ plumbing
def is_cuda(device):
    return str(device).startswith("cuda")


def family(device, what):
    return f"{what} {'hip' if is_cuda(device) else 'host'}"


def record(fam, ratio):
    WORST[fam] = max(WORST.get(fam, 0.0), float(ratio))
    return float(ratio)


@contextlib.contextmanager
def backend(device):
    """-> (the library that computes on `device`, the stream argument of its entry points)."""
    if is_cuda(device):
        with torch.cuda.device(device):
            yield nat.hip_lib, nat.current_stream_ptr(torch.device(device))
    else:
        with nat.host_mode():
            yield nat.host_lib(), None


def chunk_len(n):
    """kde_chunk_len: elements per chunk, a multiple of the tile, at most 2048 chunks."""
    q = -(-n // TARGET_CHUNKS)
    return max(-(-q // TILE), 1) * TILE


def chunks(n):
    return max(-(-n // chunk_len(n)), 1)


CANARY = 64


class Guarded:
    """`nbytes` of device memory between two 64-byte canaries (0xA5), the payload pre-filled with 0xC3."""

    def __init__(self, nbytes, device):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + 2 * CANARY,), 0xA5, dtype=torch.uint8, device=device)
        self.raw[CANARY:CANARY + self.nbytes] = 0xC3
        assert self.raw.data_ptr() % 64 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + CANARY

    def intact(self):
        r = self.raw.cpu().numpy()
        return bool((r[:CANARY] == 0xA5).all() and (r[CANARY + self.nbytes:] == 0xA5).all())

    def untouched(self):
        return bool((self.raw.cpu().numpy()[CANARY:CANARY + self.nbytes] == 0xC3).all())

    def f64(self):
        return self.raw[CANARY:CANARY + self.nbytes].cpu().numpy().view(np.float64).copy()


def workspace_bytes(lib, n_elems, C_, m):
    return int(lib.hm_kde_workspace_bytes(n_elems, C_, m))


def raw_moments(device, flat_v, flat_s, C_, c, n_elems=None, ws_delta=0, expect=nat.HM_OK):
    """hm_kde_moments on channel c of the flat (n * C_) arrays -> the 11 moments (None when `expect` is an error: then nothing was written)."""
    with backend(device) as (lib, stream):
        v = torch.tensor(flat_v, device=device) if len(flat_v) else torch.zeros(1, dtype=torch.float64, device=device)
        s = None if flat_s is None else (torch.tensor(flat_s, device=device) if len(flat_s) else torch.ones(1, dtype=torch.float64, device=device))
        n_elems = len(flat_v) if n_elems is None else n_elems
        wsb = workspace_bytes(lib, n_elems, C_, 0) + ws_delta
        ws, mom = Guarded(max(wsb, 0), device), Guarded(nat.HM_KDE_MOMENTS * 8, device)
        rc = lib.hm_kde_moments(v.data_ptr(), nat.ptr(s), n_elems, C_, c, mom.ptr, ws.ptr, wsb, stream)
        if is_cuda(device):
            torch.cuda.synchronize()
        assert rc == expect, (rc, expect)
        assert ws.intact() and mom.intact(), "a write outside moments / the workspace"
        if expect != nat.HM_OK:
            assert mom.untouched() and ws.untouched()
            return None
        return mom.f64()


def raw_evaluate(device, flat_v, flat_s, C_, c, h, scale, grid, ws_delta=0, expect=nat.HM_OK):
    """hm_kde_evaluate with the given h, scale and grid -> out (m,) (None when `expect` is an error: then nothing was written)."""
    with backend(device) as (lib, stream):
        v = torch.tensor(flat_v, device=device)
        s = None if flat_s is None else torch.tensor(flat_s, device=device)
        g = torch.tensor(np.ascontiguousarray(grid, np.float64), device=device)
        m = g.numel()
        wsb = workspace_bytes(lib, v.numel(), C_, m) + ws_delta
        if is_cuda(device):                                              # the ABI's chunking is the one restated above
            assert wsb - ws_delta == max(chunks(v.numel() // C_) * m * 8, MOM_BYTES)
        ws, out = Guarded(max(wsb, 0), device), Guarded(m * 8, device)
        rc = lib.hm_kde_evaluate(v.data_ptr(), nat.ptr(s), v.numel(), C_, c, h, scale, g.data_ptr(), m, out.ptr, ws.ptr, wsb, stream)
        if is_cuda(device):
            torch.cuda.synchronize()
        assert rc == expect, (rc, expect)
        assert ws.intact() and out.intact(), "a write outside out / the workspace"
        if expect != nat.HM_OK:
            assert out.untouched() and ws.untouched()
            return None
        return out.f64()


# ------------------------------------------------------------------------------------------------ the estimate: reference and bound
def counted(x, s):
    keep = np.isfinite(x)
    return keep if s is None else keep & (s != 0)


def sum_coefficient(n, n_counted, hip):
    if hip:
        return chunk_len(n) // TILE + -(-chunks(n) // 16) + 16 + math.log2(max(n, 2))
    return HOST_CHUNK // TILE + -(-max(n_counted, 1) // HOST_CHUNK) + math.log2(max(n, 2))


def evaluate_reference(x, s, h, scale, grid, cols=None):
    """One channel: x, s (or None) float64 (n,), grid (m,) -> dict(ref (m,) longdouble, term (m,): sum_i k_ij |t_ij| with the per-term
    coefficient k of the module docstring, tabs (m,): sum_i |t_ij|, wabs: sum|w|, counted). Blocks of grid points bound the memory."""
    keep = counted(x, s)
    xs = x[keep].astype(LD)
    w = np.ones(xs.shape, LD) if s is None else LD(1) / s[keep].astype(LD)
    hl, grid = LD(h), np.asarray(grid, np.float64)
    cols = np.arange(grid.size) if cols is None else np.asarray(cols)
    ref, term, tabs = (np.zeros(cols.size, LD) for _ in range(3))
    uu = xs / hl
    step = max(1, (1 << 22) // max(xs.size, 1))
    with np.errstate(under="ignore", over="ignore"):
        for j0 in range(0, cols.size, step):
            vv = grid[cols[j0:j0 + step]].astype(LD) / hl
            d = uu[:, None] - vv[None, :]
            t = w[:, None] * np.exp(-(d * d) / 2)
            k = np.abs(d) * (np.abs(uu)[:, None] + np.abs(vv)[None, :]) + C1 * d * d + C2
            ref[j0:j0 + step] = t.sum(0) * LD(scale)
            tabs[j0:j0 + step] = np.abs(t).sum(0) * abs(LD(scale))
            term[j0:j0 + step] = (k * np.abs(t)).sum(0) * abs(LD(scale))
    return dict(ref=ref, term=term, tabs=tabs, wabs=np.abs(w).sum(), counted=int(xs.size), n=int(x.size), scale=float(scale))


def evaluate_bound(r, hip):
    """The asserted bound of the module docstring, from evaluate_reference's sums alone."""
    coef = sum_coefficient(r["n"], r["counted"], hip)
    floor = (r["wabs"] + r["counted"] + 1) * TINY * max(abs(r["scale"]), 1.0)
    return 2 * (LD(U) * (r["term"] + coef * r["tabs"]) + E_LD * 2 * r["term"] + floor)


def restate(x, s, h, scale, grid):
    """hm_kde.hip's operation sequence in float64 NumPy: masked elements staged as (u, w) = (0, 0), a chunk's elements added one after
    the other, slice s of the 16 adding chunks s, s + 16, ..., the slices in order, times scale. (No tile is skipped: a skipped one
    adds exact zeros.)"""
    n, m = x.size, len(grid)
    L, K = chunk_len(n), chunks(n)
    keep = counted(x, s)
    with np.errstate(all="ignore"):
        u = np.zeros(K * L)
        w = np.zeros(K * L)
        u[:n] = np.where(keep, x / h, 0.0)
        w[:n] = np.where(keep, 1.0 if s is None else 1.0 / np.where(keep, s, 1.0), 0.0)
        v = np.asarray(grid, np.float64) / h
        part = np.empty((K, m))
        kb = max(1, (1 << 22) // (L * m))
        for k0 in range(0, K, kb):
            d = u[k0 * L:(k0 + kb) * L, None] - v[None, :]
            t = w[k0 * L:(k0 + kb) * L, None] * np.exp(-(d * d) * 0.5)
            part[k0:k0 + kb] = np.add.accumulate(t.reshape(-1, L, m), axis=1)[:, -1, :]
        total = np.zeros(m)
        for sl in range(16):
            a = np.zeros(m)
            for q in range(sl, K, 16):
                a = a + part[q]
            total = a if sl == 0 else total + a
    return total * scale


def restate_with_cut(x, s, h, scale, grid, cut):
    """restate() with k_kde_eval's skip rule at a given cut: per grid block of 1024 points, a tile whose counted u = x / h all lie more than
    `cut` outside the block's [min v, max v] adds nothing (masking its elements is the same thing: they are staged as w = 0)."""
    out = np.empty(len(grid))
    keep = counted(x, s)
    L = chunk_len(x.size)
    assert L == TILE, "written for chunks of one tile"
    for b0 in range(0, len(grid), BLOCK_PTS):
        cols = np.asarray(grid[b0:b0 + BLOCK_PTS], np.float64)
        v = cols / h
        xb = x.copy()
        for t0 in range(0, x.size, TILE):
            u = (x[t0:t0 + TILE] / h)[keep[t0:t0 + TILE]]
            if u.size and (u.min() > v.max() + cut or u.max() < v.min() - cut):
                xb[t0:t0 + TILE] = np.nan
        out[b0:b0 + BLOCK_PTS] = restate(xb, s, h, scale, cols)
    return out


def assert_estimate(fam, got, r, hip, what):
    """got (m,) float64 against evaluate_reference's dict: finite everywhere and inside the derived bound (which is the underflow floor
    alone where the reference is 0)."""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == r["ref"].shape, what
    assert np.isfinite(got).all(), f"{what}: a non-finite estimate"
    bound = evaluate_bound(r, hip)
    err = np.abs(got.astype(LD) - r["ref"])
    ratio = float((err / bound).max())
    record(fam, ratio)
    assert ratio <= 1.0, f"{what}: {ratio:.3f} x the derived bound at grid point {int((err / bound).argmax())}"
    return ratio


# ------------------------------------------------------------------------------------------------ the estimate: cases
def _data(seed, n, loc, sd, with_std, nan_every=0, zero_std_every=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * sd + loc
    s = rng.uniform(0.5, 2.0, n) if with_std else None
    if nan_every:
        x[5 % n::nan_every] = np.nan
    if zero_std_every and with_std:
        s[11 % n::zero_std_every] = 0.0
    return x, s


COUNTS = [1, 1023, 1024, 1025, 2_097_152, 2_097_153]
GRID_SIZES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
SUM_CHUNKS = [1, 15, 16, 17, 48, 49, 63, 64, 65, 79, 80, 81]


@functools.lru_cache(maxsize=None)
def count_case(n):
    """m = 3, C = 1. 2 097 153: chunks of two tiles, 1025 of them, the last with one element. NaN: elements [2048, 3072), the FIRST tile
    of chunk 1 (a masked tile before a live one); [4096, 6144), the whole of chunk 2; [7168, 8192), the SECOND tile of chunk 3 (a masked
    tile after a live one in the same workgroup: its accumulators must survive it). Every 997th std is 0."""
    big = n > 4096
    x, s = _data(n, n, 0.1, 0.3, with_std=n != 2_097_152, nan_every=0 if n == 1 else 101, zero_std_every=0 if n == 1 else 997)
    if n == 2_097_153:
        assert chunk_len(n) == 2048 and chunks(n) == 1025
        x[2048:3072] = np.nan
        x[4096:6144] = np.nan
        x[7168:8192] = np.nan
    if n == 2_097_152:
        assert chunk_len(n) == 1024 and chunks(n) == 2048
    h, scale, grid = (0.004 if big else 0.07), 0.37, np.array([-0.2, 0.1, 0.5])
    return x, s, 1, 0, h, scale, grid


@functools.lru_cache(maxsize=None)
def grid_case(m):
    """n = 3000 elements of C = 2, channel 1, offset data (|x / h| about 250: the |d| (|u| + |v|) term); channel 0 is a decoy of huge
    weights on the grid, which a read of the wrong channel would add."""
    n = 3000
    x, s = _data(100 + m, n, 5.0, 0.3, with_std=True, nan_every=211, zero_std_every=307)
    grid = np.linspace(4.0, 6.0, m) if m > 1 else np.array([5.1])
    xv = np.stack([np.resize(grid, n), x], axis=1).ravel()
    sv = np.stack([np.full(n, 1e-30), s], axis=1).ravel()
    return xv, sv, 2, 1, 0.02, 1.9, grid


@functools.lru_cache(maxsize=None)
def sum_case(k):
    n = k * 1024 - 5
    assert chunk_len(n) == 1024 and chunks(n) == k
    x, s = _data(200 + k, n, -0.4, 1.0, with_std=False, nan_every=1013)
    return x, s, 1, 0, 0.11, 0.013, np.linspace(-3.0, 2.5, 17)


FAR_H = 0.37
FAR_NEAREST = 37.3                                                          # the cut the far-tail test detects: any below this
FAR_TILES = ((-120.0, -100.0), (-37.5, -FAR_NEAREST), (49.0, 51.0), (100.0 + FAR_NEAREST, 137.5), (300.0, 310.0))   # in bandwidths, one tile each


@functools.lru_cache(maxsize=None)
def far_case():
    """Sorted data, five tiles and a ragged sixth, 2049 grid points on [0, 100] bandwidths: grid blocks [0, 50), [50, 100), {100}.
        tile 1, u in [-37.5, -37.3]   37.3 to 37.5 bandwidths from the grid point 0 (exp(-37.5^2 / 2) = 4e-306 is a normal number), the
                                      only elements within 38.7 of it; kept by block 0 alone, and only while the cut is at least 37.3:
                                      k_kde_eval compares the tile's nearest u with the block's nearest v
        tile 2, u in [49, 51]         the bulk, kept by blocks 0 and 1; 49 or more from 0 and from 100
        tile 3, u in [137.3, 137.5]   37.3 to 37.5 from the point 100, the only elements within 38.7 of it; kept by block 2 - and by
                                      block 1, whose points reach 99.95 - only while the cut is at least 37.3
        tiles 0, 4 and the rest       beyond 38.7 of every grid point: skipped by every block
    So every cut below 37.3 zeroes the estimates at 0 and at 100 (test_far_tail_detects_a_short_cut shows it on a NumPy model of the
    skip rule); between 37.3 and the exact 38.61 exp's result at these distances is subnormal or 0 and carries no relative accuracy.
    -> (case, the same with every element beyond 38.7 bandwidths of every grid point replaced by NaN)."""
    rng = np.random.default_rng(77)
    u = np.concatenate([np.sort(rng.uniform(lo, hi, TILE)) for lo, hi in FAR_TILES] + [np.sort(rng.uniform(320.0, 330.0, 100))])
    x = u * FAR_H
    s = rng.uniform(0.5, 2.0, x.size)
    grid = np.linspace(0.0, 100.0, 2049) * FAR_H
    du = np.abs(x[:, None] / FAR_H - grid[None, :] / FAR_H).min(1)
    gone = du > 38.7
    assert gone[:TILE].all() and gone[4 * TILE:].all() and not gone[TILE:4 * TILE].any()
    for j, tile in ((0, 1), (2048, 3)):                                       # the two ends of the grid and the one tile each of them sees
        near = np.abs(x / FAR_H - grid[j] / FAR_H)
        mine = slice(tile * TILE, (tile + 1) * TILE)
        assert FAR_NEAREST <= near[mine].min() and near[mine].max() <= 37.5 + 1e-9 and np.delete(near, mine).min() > 38.7
    x_nan = np.where(gone, np.nan, x)
    return (x, s, 1, 0, FAR_H, 0.73, grid), (x_nan, s, 1, 0, FAR_H, 0.73, grid)


@functools.lru_cache(maxsize=None)
def overflow_case():
    """h = 1e-300: the finite +-1e10 and 1e308 have an infinite x / h, contribute exp(-inf) = 0 exactly and leave no NaN."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal(1500) * 1e-300
    x[[3, 700, 1499]] = [1e10, -1e10, 1e308]
    return x, None, 1, 0, 1e-300, 0.5, np.linspace(-2e-300, 2e-300, 9)


@functools.lru_cache(maxsize=None)
def workspace_case():
    """n = 8189 (8 chunks), m = 1024: the evaluate partials are exactly the 64 KiB of the moments' partials."""
    n, m = 8189, 1024
    assert chunks(n) * m * 8 == MOM_BYTES
    x, s = _data(31, n, 0.0, 1.0, with_std=True)
    return x, s, 1, 0, 0.3, 0.2, np.linspace(-2.0, 2.0, m)


CASES = {"count": count_case, "grid": grid_case, "sum": sum_case, "far": lambda _: far_case()[0], "overflow": lambda _: overflow_case(),
         "workspace": lambda _: workspace_case()}
ALL_CASES = [("count", n) for n in COUNTS] + [("grid", m) for m in GRID_SIZES] + [("sum", k) for k in SUM_CHUNKS] + [
    ("far", None), ("overflow", None), ("workspace", None)]


def case_of(kind, key=None):
    """-> (flat values, flat stds or None, C, channel, h, scale, grid)."""
    return CASES[kind](key)


@functools.lru_cache(maxsize=None)
def reference_of(kind, key=None):
    """The long-double reference of a case: computed once, shared by every test that needs it, never modified."""
    xv, sv, C_, c, h, scale, grid = case_of(kind, key)
    return evaluate_reference(xv[c::C_], None if sv is None else sv[c::C_], h, scale, grid)


def check_estimate(device, kind, key=None):
    xv, sv, C_, c, h, scale, grid = case_of(kind, key)
    got = raw_evaluate(device, xv, sv, C_, c, h, scale, grid)
    return got, assert_estimate(family(device, f"evaluate {kind}"), got, reference_of(kind, key), is_cuda(device), f"{kind} {key}")


def check_far_tail(device):
    """The cut. The estimates at the grid's two ends come from pairs 37.3 to 37.5 bandwidths apart alone: positive, about 1e-301, inside
    the relative bound - any cut below 37.3 drops them. Elements beyond 38.7 of every grid point replaced by NaN: the same bits."""
    got, _ = check_estimate(device, "far")
    r = reference_of("far")
    ref = r["ref"].astype(np.float64)
    for j in (0, 2048):
        assert 1e-304 < ref[j] < 1e-295 and got[j] > 0.0, (j, ref[j], got[j])
        assert abs(LD(got[j]) - r["ref"][j]) <= 1e-11 * r["ref"][j], (j, got[j], ref[j])       # (implied by the bound: about 3e-13)
    assert ref[1024] > 1e-3                                                                    # the bulk, mid-grid
    xv, sv, C_, c, h, scale, grid = far_case()[1]
    again = raw_evaluate(device, xv, sv, C_, c, h, scale, grid)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), "masking the elements beyond the cut changed bits"


def check_overflow(device):
    got, _ = check_estimate(device, "overflow")
    assert (got > 0).all()


def check_workspace_size(device):
    """n = 8189 (8 chunks), m = 1024: the evaluate partials are exactly the moments' 64 KiB, so hm_kde_workspace_bytes is the minimum of
    BOTH entries (the host build needs none: 0, and a negative size is its HM_EINVAL). One byte less: HM_EINVAL, nothing written."""
    x, s, C_, c, h, scale, grid = workspace_case()
    with backend(device) as (lib, _):
        wsb = workspace_bytes(lib, x.size, C_, len(grid))
    assert wsb == (MOM_BYTES if is_cuda(device) else 0)
    check_estimate(device, "workspace")                                   # (raw_evaluate passes exactly hm_kde_workspace_bytes)
    assert raw_moments(device, x, s, C_, c) is not None
    assert raw_evaluate(device, x, s, C_, c, h, scale, grid, ws_delta=-1, expect=nat.HM_EINVAL) is None
    assert raw_moments(device, x, s, C_, c, ws_delta=-1, expect=nat.HM_EINVAL) is None


# ------------------------------------------------------------------------------------------------ moments
MOMENT_COUNTS = [0, 1, 255, 256, 257, 131_071, 131_072, 131_073]             # 131 072: one pass of 512 workgroups of 256 lanes
MOMENT_CHANNELS = [1, 3, 5]
STD_KINDS = ["none", "plain", "special", "negative", "mixed"]


@functools.lru_cache(maxsize=None)
def moment_case(n, C_, kind):
    """(n, C_) values with NaN, +inf, -inf among them; stds by kind: none; plain (positive); special (+0 and -0: not counted; inf:
    counted with w = 0; NaN and a subnormal: counted, flagged non-finite); negative (all below 0); mixed (both signs)."""
    rng = np.random.default_rng(1000 * C_ + n % 977 + 7 * STD_KINDS.index(kind))
    x = rng.standard_normal((n, C_)) * 0.5 + np.arange(C_) * 3.0 - 2.0
    pick = rng.random((n, C_))
    x[pick < 0.02] = np.nan
    x[(pick >= 0.02) & (pick < 0.03)] = np.inf
    x[(pick >= 0.03) & (pick < 0.04)] = -np.inf
    if kind == "none":
        return x.ravel(), None
    s = rng.uniform(0.25, 4.0, (n, C_))
    if kind == "negative":
        s = -s
    if kind == "mixed":
        s[rng.random((n, C_)) < 0.4] *= -1.0
    if kind == "special":
        q = rng.random((n, C_))
        for lo, val in ((0.00, 0.0), (0.03, -0.0), (0.06, np.inf), (0.09, np.nan), (0.10, 5e-324 * 1000)):
            s[(q >= lo) & (q < lo + (0.03 if val == 0 or val == np.inf else 0.01))] = val
        if n >= 255:                                                       # one channel without non-finite weights: its sums stay finite
            s[..., 0] = np.where(np.isnan(s[..., 0]) | (np.abs(s[..., 0]) < 1e-300) & (s[..., 0] != 0), 1.5, s[..., 0])
    return x.ravel(), s.ravel()


def exact_sum(a):
    """The sum of a longdouble array as a longdouble: exact (math.fsum over float64 halves, then the remainder) where every element is
    finite, IEEE's inf / NaN otherwise."""
    a = np.asarray(a, LD)
    if not np.isfinite(a).all():
        with np.errstate(invalid="ignore"):
            return a.sum()
    hi = a.astype(np.float64)
    lo = (a - hi).astype(np.float64)
    parts = hi.tolist() + lo.tolist()
    r = math.fsum(parts)
    return LD(r) + LD(math.fsum(parts + [-r]))


def moments_reference(x, s):
    """One channel -> (ref (11,) longdouble, bound terms dict)."""
    keep = counted(x, s)
    xs = x[keep]
    with np.errstate(all="ignore"):
        w = np.ones(xs.shape) if s is None else 1.0 / s[keep]
        xl, wl = xs.astype(LD), w.astype(LD)
        ref = np.zeros(11, LD)
        ref[0] = xs.size
        ref[1], ref[2], ref[3] = exact_sum(wl), exact_sum(wl * wl), exact_sum(wl * xl)
        ref[4], ref[5] = (xs.min(), xs.max()) if xs.size else (np.inf, -np.inf)
        ref[6], ref[7], ref[8] = (~np.isfinite(w)).sum(), (w > 0).sum(), (w < 0).sum()
        ref[9] = ref[3] / ref[1]
        d = xl - ref[9]
        ref[10] = exact_sum(wl * d * d)
        sums = dict(w=np.abs(wl).sum(), w2=(wl * wl).sum(), wx=np.abs(wl * xl).sum(), wd=np.abs(wl * d).sum(), wd2=np.abs(wl * d * d).sum())
    return ref, sums


def moments_bound(ref, sums, n, hip):
    """-> bound (11,) longdouble; 0 for the exact entries."""
    D = (-(-n // MOM_LANES) + 23) if hip else (-(-n // HOST_SLICES) + HOST_SLICES)
    u = LD(U)
    b = np.zeros(11, LD)
    with np.errstate(all="ignore"):
        b[1], b[2], b[3] = D * u * sums["w"], (D + 1) * u * sums["w2"], (D + 1) * u * sums["wx"]
        db = b[3] / abs(ref[1]) + abs(ref[3]) * b[1] / (ref[1] * ref[1]) + u * abs(ref[9])
        b[9] = db
        b[10] = (D + 4) * u * sums["wd2"] + 2 * db * sums["wd"] + db * db * sums["w"]
    return 2 * b + 2 * E_LD * np.abs(ref)


EXACT = (0, 4, 5, 6, 7, 8)


def check_moments(device, n, C_, kind):
    xv, sv = moment_case(n, C_, kind)
    worst = 0.0
    for c in range(C_):
        got = raw_moments(device, xv, sv, C_, c, n_elems=n * C_)
        ref, sums = moments_reference(xv[c::C_], None if sv is None else sv[c::C_])
        what = f"n={n} C={C_} c={c} {kind}"
        for k in EXACT:
            assert got[k] == float(ref[k]), f"{what}: moment {k}: {got[k]} != {ref[k]}"
        if ref[0] == 0:                                                  # nothing counted (n = 0, or every element masked)
            assert got[0] == 0 and got[4] == np.inf and got[5] == -np.inf and np.isnan(got[9]), what
            assert got[1] == 0 and got[2] == 0 and got[3] == 0 and got[10] == 0, what
            continue
        bound = moments_bound(ref, sums, n, is_cuda(device))
        for k in (1, 2, 3, 9, 10):
            if not np.isfinite(ref[k]):
                r64 = float(ref[k])
                assert (np.isnan(got[k]) and np.isnan(r64)) or got[k] == r64, f"{what}: moment {k}: {got[k]} for {r64}"
                continue
            assert np.isfinite(bound[k]) and np.isfinite(got[k]), f"{what}: moment {k}: a finite reference {float(ref[k])} without a finite bound"
            err = abs(LD(got[k]) - ref[k])
            if bound[k] == 0:
                assert err == 0, f"{what}: moment {k}"
                continue
            worst = max(worst, record(family(device, "moments"), err / bound[k]))
            assert err <= bound[k], f"{what}: moment {k}: {float(err / bound[k]):.3f} x the bound ({got[k]} for {float(ref[k])})"
    return worst


def check_moment_flags_present():
    """The 'special' set really holds every kind of std the issue lists, and the 'negative' / 'mixed' sets are what they say."""
    xv, sv = moment_case(131_073, 3, "special")
    assert (sv == 0).any() and np.signbit(sv[sv == 0]).any() and not np.signbit(sv[sv == 0]).all()
    assert np.isinf(sv).any() and np.isnan(sv).any() and ((sv > 0) & (sv < 2.3e-308)).any()
    assert np.isnan(xv).any() and np.isposinf(xv).any() and np.isneginf(xv).any()
    assert (moment_case(257, 3, "negative")[1] < 0).all()
    mixed = moment_case(257, 3, "mixed")[1]
    assert (mixed < 0).any() and (mixed > 0).any()


# ------------------------------------------------------------------------------------------------ the tests, on the host build
HOST = "cpu"


@pytest.mark.parametrize("kind,key", ALL_CASES)
def test_restatement_within_bound(kind, key):
    """Without any kernel: the float64 restatement of the device's sequence against the long-double reference, inside the HIP bound."""
    xv, sv, C_, c, h, scale, grid = case_of(kind, key)
    got = restate(xv[c::C_], None if sv is None else sv[c::C_], h, scale, grid)
    assert_estimate(f"evaluate {kind} restatement", got, reference_of(kind, key), True, f"{kind} {key}")


def test_restatement_far_tail_masked_bits():
    a, b = far_case()
    ra = restate(a[0], a[1], a[4], a[5], a[6])
    rb = restate(b[0], b[1], b[4], b[5], b[6])
    assert np.array_equal(ra.view(np.uint64), rb.view(np.uint64))


@pytest.mark.parametrize("cut,detected", [(10.0, True), (30.0, True), (36.0, True), (37.2, True), (37.6, False), (38.7, False)])
def test_far_tail_detects_a_short_cut(cut, detected):
    """What the far-tail case can see, on a NumPy model of k_kde_eval's skip rule: every cut below 37.3 leaves the bound at both ends of
    the grid; the exact cut, and any down to the tiles' farthest element, gives the bits of no skipping at all."""
    x, s, _, _, h, scale, grid = far_case()[0]
    got = restate_with_cut(x, s, h, scale, grid, cut)
    r = reference_of("far")
    ratio = np.abs(got.astype(LD) - r["ref"]) / evaluate_bound(r, True)
    if detected:
        assert ratio[0] > 1e6 and ratio[2048] > 1e6 and got[0] == 0.0 and got[2048] == 0.0
    else:
        assert np.array_equal(got.view(np.uint64), restate(x, s, h, scale, grid).view(np.uint64)) and ratio.max() <= 1.0


SMALL_CASES = [("count", n) for n in COUNTS if n <= 4096] + [("grid", m) for m in GRID_SIZES] + [("sum", 1), ("far", None), ("overflow", None)]


@pytest.mark.parametrize("kind,key", SMALL_CASES)
def test_reference_against_mpmath(kind, key):
    """The long-double reference against mpmath at 40 digits, within its stated error (the per-term expression with 2^-64): every case
    of at most 4096 elements, and the far tail (5220) at its two ends, where the exponent is largest."""
    import mpmath
    xv, sv, C_, c, h, scale, grid = case_of(kind, key)
    x, s = xv[c::C_], None if sv is None else sv[c::C_]
    keep = counted(x, s)
    m = len(grid)
    cols = np.unique(np.linspace(0, m - 1, max(1, min(m, 12_000 // max(int(keep.sum()), 1)))).round().astype(int))
    r = evaluate_reference(x, s, h, scale, grid, cols)
    with mpmath.workdps(40):
        mh, two = mpmath.mpf(h), mpmath.mpf(2)
        xs = [mpmath.mpf(float(v)) for v in x[keep]]
        ws = [mpmath.mpf(1) if s is None else 1 / mpmath.mpf(float(v)) for v in (x[keep] if s is None else s[keep])]
        for k, j in enumerate(cols):
            y = mpmath.mpf(float(grid[j]))
            want = mpmath.fsum(w * mpmath.exp(-(((xi - y) / mh) ** 2) / two) for xi, w in zip(xs, ws)) * mpmath.mpf(scale)
            hi = float(r["ref"][k])
            got = mpmath.mpf(hi) + mpmath.mpf(float(r["ref"][k] - LD(hi)))
            allowed = 4 * float(E_LD) * (float(r["term"][k]) + 16 * float(r["tabs"][k])) + float(TINY) * (float(r["wabs"]) + 1)
            assert abs(got - want) <= allowed, (kind, key, j, got, want)


@pytest.mark.parametrize("n", COUNTS)
def test_host_element_counts(n):
    check_estimate(HOST, "count", n)


@pytest.mark.parametrize("m", GRID_SIZES)
def test_host_grid_sizes(m):
    check_estimate(HOST, "grid", m)


@pytest.mark.parametrize("k", SUM_CHUNKS)
def test_host_chunk_counts(k):
    check_estimate(HOST, "sum", k)


def test_host_far_tail():
    check_far_tail(HOST)


def test_host_overflowing_quotient():
    check_overflow(HOST)


def test_host_workspace_size():
    check_workspace_size(HOST)


@pytest.mark.parametrize("kind", STD_KINDS)
@pytest.mark.parametrize("C_", MOMENT_CHANNELS)
@pytest.mark.parametrize("n", MOMENT_COUNTS)
def test_host_moments(n, C_, kind):
    check_moments(HOST, n, C_, kind)


def test_moment_cases_hold_every_special():
    check_moment_flags_present()
