"""The all-pairs linearity distributions - hm_pairs_histogram / hm_pairs_minmax (csrc/hm_stats_hist.hip: k_pairs_hist, k_pairs_minmax,
k_pairs_minmax_final, k_hist_final), engine.pairs_histogram and ExposureSeries.process_linearity_distribution - on the HOST build
(csrc_host/hm_host.cpp). The checks are functions of a device name: tests/test_gpu_pairs_hist.py runs the same ones on the MI355X.

Reference (diff_reference)
    The difference images and their stds in NumPy float64, k_difference's expressions written out: scale = m y; a = x - scale;
    r = a / scale; as = sqrt(xs xs + (m ys)(m ys)); rs = sqrt(u1 u1 + u2 u2) with u1 = xs / (m y), u2 = (ys x) / (m (y y)). Thresholds
    are np.where(outside, NaN, .) on value and std before. NumPy rounds every operation once and fuses nothing - the library is built
    with -ffp-contract=off - so these are the bits both builds bin and weigh. Then hist_reference / assert_hist of
    tests/test_stats_limits_host.py per (pair, kind, channel).
Asserted
    Unweighted counts equal and their sum equals the in-range count; edges bit-equal to np.linspace; empty bins exactly 0.0; NaN / inf
    patterns equal; every other weighted bin within (k_b + 2) u sum_b |1 / std|, u = 2^-53 (the weights are the same float64 bits on both
    sides: one rounding per reciprocal, k_b - 1 additions in any order, one for the reference's conversion). The fused result equals
    the unfused path of the same backend (compute_difference + channel_histogram): exactly when unweighted, within twice the bound when
    weighted (each side is within the bound of the reference). hm_pairs_minmax is exact.
Sizes that come from the kernel's constants (hm_stats_hist.hip)
    A launch of np pairs gives every pair wpp = HM_PAIRS_MAX / np waves and runs min(ceil(n / (64 wpp)) rounded up to a multiple of 12,
    kPairsHistBlocks x per_cu) workgroups, each taking wpp 64-element chunks per sweep; kPairsHistBlocks = 252, per_cu = min(160 KiB /
    LDS of the workgroup, 32 / (np wpp), kPairsHistMaxPerCU = 4), LDS of the workgroup = np x 2 x C x bins x 8 bytes. FULL_SWEEP is one
    sweep of a 3-pair, 32-bin, C = 3 launch (504 workgroups of 15 waves); RAGGED is three such sweeps and 37 more pixels. Pairs per launch = min(HM_PAIRS_MAX, 160 KiB / (2 x C x bins x 8)): SPLIT_BINS is
    the smallest bin count at which three pairs at C = 3 no longer fit one launch.

Every check records its largest error as a fraction of its bound; the module prints the maxima at its end."""
import ctypes as C

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd.exposure_series import ExposurePair, ExposureSeries
from camera_linearity_amd.image_set import ImageSet

import test_stats_limits_host as sl
from test_stats_limits_host import LD, U, T, backend, eng, family, record, hist_reference, assert_hist, edge_inputs, bin_index
from test_stats_limits_host import report_observed_maxima  # noqa: F401  (prints the observed maxima after this module too)

LDS_BYTES = 160 * 1024
BLOCKS, PER_CU_MAX, CHUNK = 252, 4, 64                      # kPairsHistBlocks, kPairsHistMaxPerCU, elements per workgroup and sweep


def pairs_per_launch(bins, C_):
    return min(nat.HM_PAIRS_MAX, LDS_BYTES // (2 * C_ * bins * 8))


def sweep_elements(np_, bins, C_):
    wpp = nat.HM_PAIRS_MAX // np_
    per_cu = max(1, min(LDS_BYTES // (np_ * 2 * C_ * bins * 8), 32 // (np_ * wpp), PER_CU_MAX))
    return BLOCKS * per_cu * wpp * CHUNK


FULL_SWEEP = sweep_elements(3, 32, 3) // 3                  # pixels (C = 3): 53 760
RAGGED = 3 * FULL_SWEEP + 37
SPLIT_BINS = next(b for b in range(1, nat.HM_PAIRS_HIST_MAX_BINS + 1) if pairs_per_launch(b, 3) < 3)


def test_sizes_follow_the_kernel_constants():
    assert FULL_SWEEP * 3 == 504 * 5 * 64 and RAGGED * 3 < 1_500_000
    assert SPLIT_BINS == 1138 and pairs_per_launch(SPLIT_BINS, 3) == 2 and pairs_per_launch(SPLIT_BINS - 1, 3) == 3
    assert pairs_per_launch(256, 3) == 13 and pairs_per_launch(2048, 4) == 1 and pairs_per_launch(1, 1) == nat.HM_PAIRS_MAX


# ------------------------------------------------------------------------------------------------ reference
def diff_reference(x, xs, y, ys, m, lower=None, upper=None):
    """(..., C) float64 arrays -> (a, as, r, rs); as / rs None without stds."""
    if lower is not None:
        lo, hi = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
        ox, oy = (x < lo) | (x > hi), (y < lo) | (y > hi)
        x, y = np.where(ox, np.nan, x), np.where(oy, np.nan, y)
        if xs is not None:
            xs, ys = np.where(ox, np.nan, xs), np.where(oy, np.nan, ys)
    with np.errstate(all="ignore"):
        scale = m * y
        a = x - scale
        r = a / scale
        if xs is None:
            return a, None, r, None
        m1 = m * ys
        as_ = np.sqrt(xs * xs + m1 * m1)
        u1 = xs / (m * y)
        u2 = (ys * x) / (m * (y * y))
        return a, as_, r, np.sqrt(u1 * u1 + u2 * u2)


def default_range(x, s):
    """np.histogram's default range of the counted values with its two rules."""
    xs = x[sl.counted(x, s)]
    lo, hi = (float(xs.min()), float(xs.max())) if xs.size else (0.0, 1.0)
    return (lo - 0.5, hi + 0.5) if lo == hi else (lo, hi)


# ------------------------------------------------------------------------------------------------ raw calls
class Args:
    """The host-side argument arrays of one call; tensors are kept alive here."""

    def __init__(self, device, frames, stds, pairs, tensors=None, std_tensors=None):
        self.v = tensors if tensors is not None else [T(f, device) for f in frames]
        self.s = std_tensors if std_tensors is not None else (None if stds is None else [T(s, device) for s in stds])
        self.P = len(pairs)
        self.vp = C.cast((C.c_void_p * len(self.v))(*[t.data_ptr() for t in self.v]), C.POINTER(C.c_void_p))
        self.sp = None if self.s is None else C.cast((C.c_void_p * len(self.s))(*[t.data_ptr() for t in self.s]), C.POINTER(C.c_void_p))
        self.pi = (C.c_int32 * self.P)(*[p[0] for p in pairs])
        self.pj = (C.c_int32 * self.P)(*[p[1] for p in pairs])
        self.pm = (C.c_double * self.P)(*[p[2] for p in pairs])


def limits(thr, C_):
    if thr is None:
        return None, None
    return (C.c_double * C_)(*thr[0]), (C.c_double * C_)(*thr[1])


def raw_minmax(device, frames, stds, pairs, C_, thr=None, expect=nat.HM_OK, args=None):
    with backend(device) as (lib, stream):
        a = args or Args(device, frames, stds, pairs)
        lo, hi = limits(thr, C_)
        out = torch.full((a.P * 2 * C_ * 2,), float("nan"), dtype=torch.float64, device=device)
        ws = torch.empty(max(8, lib.hm_pairs_histogram_workspace_bytes(a.P, 1, C_) // 8), dtype=torch.float64, device=device)
        rc = lib.hm_pairs_minmax(a.vp, a.sp, len(a.v), a.pi, a.pj, a.pm, a.P, a.v[0].numel(), C_, lo, hi, out.data_ptr(), ws.data_ptr(), stream)
        assert rc == expect, (rc, expect)
        return out.cpu().numpy().reshape(a.P, 2, C_, 2)


def raw_hist(device, frames, stds, pairs, C_, mask, bins, edges, thr=None, prefill=float("nan"), expect=nat.HM_OK, args=None):
    """hm_pairs_histogram called directly -> out (P, 2, C, bins) over a `prefill`ed buffer (left untouched when `expect` is an error)."""
    with backend(device) as (lib, stream):
        a = args or Args(device, frames, stds, pairs)
        lo, hi = limits(thr, C_)
        e = T(edges, device)
        nb = max(1, min(bins, 4096))
        out = torch.full((a.P * 2 * C_ * nb,), prefill, dtype=torch.float64, device=device)
        ws = torch.empty(max(8, lib.hm_pairs_histogram_workspace_bytes(a.P, bins, C_) // 8), dtype=torch.float64, device=device)
        rc = lib.hm_pairs_histogram(a.vp, a.sp, len(a.v), a.pi, a.pj, a.pm, a.P, a.v[0].numel(), C_, mask, lo, hi, e.data_ptr(), bins,
                                    out.data_ptr(), ws.data_ptr(), stream)
        assert rc == expect, (rc, expect)
        return out.cpu().numpy().reshape(a.P, 2, C_, nb)


def linspace_edges(ranges, bins):
    """ranges (P, 2, C, 2) -> edges (P, 2, C, bins + 1)."""
    e = np.empty(ranges.shape[:3] + (bins + 1,))
    for idx in np.ndindex(*ranges.shape[:3]):
        e[idx] = np.linspace(ranges[idx][0], ranges[idx][1], bins + 1)
    return e


# ------------------------------------------------------------------------------------------------ the check
def check_pairs(device, frames, stds, pairs, bins, rng=None, mask=None, thr=None, unfused=True, offset=False, what="pairs"):
    """frames / stds: lists of (npix, C) arrays; pairs [(i, j, multiplier)]. The raw ABI: min / max exact, then the histograms on the
    given range (or every (pair, kind, channel)'s default range) against the reference and against the unfused path of the backend.
    offset: the device buffers start 8 bytes past a 16-byte boundary."""
    C_ = frames[0].shape[-1]
    mask = (1 << C_) - 1 if mask is None else mask
    weighted = stds is not None
    fam = family(device, "pairs histogram")
    put = (lambda a: sl.offset_by_8(a.ravel(), device)) if offset else (lambda a: T(a.ravel(), device))
    with backend(device):
        args = Args(device, None, None, pairs, tensors=[put(f) for f in frames], std_tensors=[put(s) for s in stds] if weighted else None)
    before = [t.clone() for t in args.v + (args.s or [])]
    mm = raw_minmax(device, None, None, pairs, C_, thr, args=args)
    refs = []
    ranges = np.empty((len(pairs), 2, C_, 2))
    for p, (i, j, m) in enumerate(pairs):
        d = diff_reference(frames[i], stds[i] if weighted else None, frames[j], stds[j] if weighted else None, m,
                           None if thr is None else thr[0], None if thr is None else thr[1])
        refs.append(d)
        for k in range(2):
            for c in range(C_):
                x, s = d[2 * k][:, c], d[2 * k + 1][:, c] if weighted else None
                xs = x[sl.counted(x, s)]
                want = (xs.min(), xs.max()) if xs.size else (np.inf, -np.inf)
                assert mm[p, k, c, 0] == want[0] and mm[p, k, c, 1] == want[1], (what, p, k, c, mm[p, k, c], want)
                ranges[p, k, c] = default_range(x, s) if rng is None else rng
    edges = linspace_edges(ranges, bins)
    got = raw_hist(device, None, None, pairs, C_, mask, bins, edges, thr, args=args)
    for t, b in zip(args.v + (args.s or []), before):
        assert torch.equal(t.view(torch.int64), b.view(torch.int64)), f"{what}: a frame was modified"
    worst = 0.0
    for p, pair in enumerate(pairs):
        d = refs[p]
        images = unfused_images(device, args, pair, C_, thr) if unfused else None
        for k in range(2):
            for c in range(C_):
                if not (mask >> c) & 1:
                    assert np.all(got[p, k, c] == 0.0), f"{what}: channel {c} outside the mask is not 0.0"
                    continue
                x, s = d[2 * k][:, c], d[2 * k + 1][:, c] if weighted else None
                ref = hist_reference(x, s, bins, tuple(ranges[p, k, c]))
                h = got[p, k, c] if weighted else got[p, k, c].astype(np.int64)
                assert weighted or np.array_equal(h, got[p, k, c])                      # counts are whole numbers
                label = f"{what}: pair {p} kind {k} channel {c}"
                worst = max(worst, assert_hist(fam, h, edges[p, k, c], ref, weighted, label))
                if unfused:
                    check_unfused(device, images[k], c, bins, tuple(ranges[p, k, c]), h, ref, label)
    return got, worst


def unfused_images(device, args, pair, C_, thr):
    """compute_difference of the same backend on (thresholded copies of) the pair's frames -> ((abs, abs std), (rel, rel std))."""
    i, j, m = pair
    ops = [args.v[i].clone(), None if args.s is None else args.s[i].clone(), args.v[j].clone(), None if args.s is None else args.s[j].clone()]
    ops = [None if o is None else o.view(-1, C_) for o in ops]
    if thr is not None:
        eng(device, "apply_thresholds_", ops[0], ops[1], list(thr[0]), list(thr[1]))
        eng(device, "apply_thresholds_", ops[2], ops[3], list(thr[0]), list(thr[1]))
    ad, ads, rd, rds = eng(device, "compute_difference", ops[0], ops[1], ops[2], ops[3], m)
    return (ad, ads), (rd, rds)


def check_unfused(device, image, c, bins, rng, fused, ref, what):
    """channel_histogram of the same backend on a difference image: equal when unweighted, within twice the bound when weighted."""
    val, std = image
    h, e = eng(device, "channel_histogram", val, std, bins, rng, [c])[c]
    assert np.array_equal(e, ref["edges"])
    if std is None:
        assert np.array_equal(h, fused), f"{what}: fused != unfused"
        return
    np.testing.assert_array_equal(np.isnan(h), np.isnan(fused))
    np.testing.assert_array_equal(np.isinf(h), np.isinf(fused))
    fin = np.isfinite(ref["wsum"]) & (ref["k"] > 0) & np.isfinite(ref["wabs"]) & (ref["wabs"] > 0)
    if fin.any():
        worst = record(family(device, "pairs fused - unfused"), np.abs(h[fin].astype(LD) - fused[fin].astype(LD)),
                       2 * (ref["k"][fin] + 2) * LD(U) * ref["wabs"][fin])
        assert worst <= 1.0, f"{what}: fused - unfused {worst:.3f} x twice the bound"


# ------------------------------------------------------------------------------------------------ data
def stack(seed, n_frames, npix, C_, specials=True, ratio=1.5):
    """Near-linear frames: frame i = scene x t_i x (1 + 1 % noise), t_i = ratio^i scaled so the last frame stays below 1; stds around 1 % of
    the value. With `specials`: NaN and +-inf in some values, zeros (the relative difference against y = 0 is non-finite), std pairs of 0 and
    stds of inf. -> frames, stds, exposures."""
    rng = np.random.default_rng(seed)
    scene = 0.1 + 0.8 * rng.random((npix, C_))
    t = ratio ** np.arange(n_frames, dtype=np.float64)
    t /= t[-1]
    frames = [scene * ti * (1 + 0.01 * rng.standard_normal((npix, C_))) for ti in t]
    stds = [0.002 + 0.01 * f * rng.random((npix, C_)) for f in frames]
    if specials:
        n = npix * C_
        m = max(1, n // 60)
        for f, s in zip(frames, stds):
            for val in (np.nan, np.inf, -np.inf, 0.0):
                f.reshape(-1)[rng.integers(0, n, m)] = val
            s.reshape(-1)[rng.integers(0, n, m)] = np.inf
        z = rng.integers(0, n, m)                                           # both stds 0 at the same elements: the difference stds are 0
        for s in stds:
            s.reshape(-1)[z] = 0.0
    return frames, stds, t


def all_pairs(t, limit=None):
    pairs = [(i, j, float(t[i] / t[j])) for i in range(len(t)) for j in range(len(t)) if i < j]
    return pairs if limit is None else pairs[:limit]


# ------------------------------------------------------------------------------------------------ cases
SIZES = [("1x1", 1), ("5x7", 35), ("full sweep", FULL_SWEEP), ("ragged", RAGGED)]


def check_sizes(device, npix, C_, use_std):
    if npix >= FULL_SWEEP and C_ != 3:
        npix = npix * 3 // C_ + (1 if npix == RAGGED else 0)               # the same element counts for the other channel counts
    frames, stds, t = stack(10 * npix + C_, 2 if npix == 35 else 3, npix, C_, specials=npix > 1)
    check_pairs(device, frames, stds if use_std else None, all_pairs(t), 32, None if npix > 1 else (-1.0, 1.0), what=f"{npix} px C={C_}")


def check_masks(device, use_std):
    frames, stds, t = stack(5, 3, 411, 4)
    for mask in (0b0001, 0b1010, 0b0110, 0b0000):
        check_pairs(device, frames, stds if use_std else None, all_pairs(t), 16, (-0.05, 0.05), mask=mask, unfused=False, what=f"mask {mask:04b}")
    frames, stds, t = stack(6, 2, 200, 2)
    check_pairs(device, frames, stds if use_std else None, all_pairs(t), 16, (-0.05, 0.05), mask=0b10, what="mask 10 of C=2")


def check_seven_frames(device, use_std):
    """All 21 pairs of 7 frames: more than HM_PAIRS_MAX, so several launches of either entry point."""
    frames, stds, t = stack(7, 7, 333, 3)
    pairs = all_pairs(t)
    assert len(pairs) == 21 > nat.HM_PAIRS_MAX
    check_pairs(device, frames, stds if use_std else None, pairs, 64, None, what="7 frames, 21 pairs")


def check_thirty_two_frames(device, use_std):
    """32 frames (HM_MAX_FRAMES), 16 pairs that share frames: frame 31 against 0..7, frame 0 against 24..30, and (5, 5)."""
    frames, stds, t = stack(32, 32, 70, 3, ratio=1.05)
    pairs = [(i, 31, float(t[i] / t[31])) for i in range(8)] + [(0, j, float(t[0] / t[j])) for j in range(24, 31)] + [(5, 5, 1.0)]
    assert len(pairs) == 16
    check_pairs(device, frames, stds if use_std else None, pairs, 16, (-0.3, 0.3), what="32 frames")


BINS = [(1, 3), (2, 3), (255, 3), (256, 3), (257, 3), (SPLIT_BINS, 3), (2048, 4)]


def check_bins(device, bins, C_, use_std):
    frames, stds, t = stack(bins + C_, 3, 2999 if bins < 1000 else 9000, C_)
    check_pairs(device, frames, stds if use_std else None, all_pairs(t), bins, (-0.04, 0.04), unfused=bins <= 257, what=f"bins={bins} C={C_}")


def check_above_limit(device):
    frames, _, t = stack(3, 2, 8, 3, specials=False)
    pairs = all_pairs(t)
    bins = nat.HM_PAIRS_HIST_MAX_BINS + 1
    edges = linspace_edges(np.tile([0.0, 1.0], (1, 2, 3, 1)), bins)
    out = raw_hist(device, [f.ravel() for f in frames], None, pairs, 3, 7, bins, edges, prefill=-7.0, expect=nat.HM_EINVAL)
    assert np.all(out == -7.0)
    with pytest.raises(ValueError):
        eng(device, "pairs_histogram", [T(f, device) for f in frames], None, pairs, bins, (0.0, 1.0), [0])


EDGE_SETS = [(-0.3, 0.7, 257, 3), (0.1, 0.9, 32, 3), (-0.125, 0.25, 255, 1), (1e-3, 3e-3, 2048, 4)]


def edge_case(lo, hi, bins, C_, kind):
    """kind 0: x = the edge inputs, y = 0: a = x exactly, r non-finite. kind 1: y = 1, multiplier 1, x = fl(1 + e): r = x - 1 exactly."""
    e = np.concatenate([edge_inputs(lo, hi, bins), [lo - 1.0, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), hi + 1.0, hi, hi]])
    rng = np.random.default_rng(bins + kind)
    e = np.concatenate([e, rng.choice(e, (-e.size) % C_)])
    rng.shuffle(e)
    x = e if kind == 0 else 1.0 + e
    y = np.zeros_like(x) if kind == 0 else np.ones_like(x)
    return x.reshape(-1, C_), y.reshape(-1, C_), rng


def uncorrected_misses(values, lo, hi, bins):
    """How many of the in-range values the index int((x - lo) * (bins / (hi - lo))) puts in another bin than the edges do."""
    v = values[(values >= lo) & (values <= hi)]
    raw = ((v - lo) * (bins / (hi - lo))).astype(np.int64)
    return int((raw != bin_index(np.linspace(lo, hi, bins + 1), v)).sum())


@pytest.mark.parametrize("lo,hi,bins,C_", EDGE_SETS)
@pytest.mark.parametrize("kind", [0, 1])
def test_edge_cases_need_the_corrections(lo, hi, bins, C_, kind):
    """The precondition of check_edges: the difference image that is binned is exactly the edge inputs (kind 0) or within one ulp(1) of
    them (kind 1), and the uncorrected index formula puts at least one of its values in another bin."""
    x, y, _ = edge_case(lo, hi, bins, C_, kind)
    a, _, r, _ = diff_reference(x, None, y, None, 1.0)
    if kind == 0:
        binned = a
        assert np.array_equal(a, x) and not np.isfinite(r).any()
    else:
        binned = r
        assert np.array_equal(r, x - 1.0) and np.array_equal(a, r)
    assert uncorrected_misses(binned.ravel(), lo, hi, bins) >= 1


def check_edges(device, lo, hi, bins, C_, kind, use_std):
    x, y, rng = edge_case(lo, hi, bins, C_, kind)
    stds = [0.05 + rng.random(x.shape), 0.05 + rng.random(x.shape)] if use_std else None
    got, _ = check_pairs(device, [x, y], stds, [(0, 1, 1.0)], bins, (lo, hi), what=f"edge values ({lo}, {hi}, {bins}) kind {kind}")
    if kind == 0:
        assert np.all(got[0, 1] == 0.0)                                     # y = 0: every relative difference is non-finite


def check_specials(device):
    """NaN / +-inf in either frame, y = 0 beside finite x, both stds 0, std = inf - one element each, then a bulk of ordinary ones."""
    x = np.array([np.nan, 0.2, np.inf, 0.2, -np.inf, 0.2, 0.2, 0.25, 0.3, 0.2, 0.22, 0.21], np.float64).reshape(-1, 1)
    y = np.array([0.3, np.nan, 0.3, np.inf, 0.3, -np.inf, 0.0, 0.35, 0.4, 0.3, 0.31, 0.3], np.float64).reshape(-1, 1)
    sx = np.array([.01, .01, .01, .01, .01, .01, .01, 0.0, np.inf, .01, .02, np.nan], np.float64).reshape(-1, 1)
    sy = np.array([.01, .01, .01, .01, .01, .01, .01, 0.0, .01, np.inf, .02, .01], np.float64).reshape(-1, 1)
    a, as_, r, rs = diff_reference(x, sx, y, sy, 0.7)
    assert np.isfinite(a[6, 0]) and not np.isfinite(r[6, 0])               # y = 0 beside a finite x: absolute counted, relative skipped
    assert as_[7, 0] == 0.0 and rs[7, 0] == 0.0 and np.isinf(as_[8, 0]) and np.isinf(as_[9, 0]) and np.isnan(as_[11, 0])
    for stds in (None, [sx, sy]):
        check_pairs(device, [x, y], stds, [(0, 1, 0.7)], 8, (-1.0, 1.0), what="special values")
        check_pairs(device, [x, y], stds, [(0, 1, 0.7)], 8, None, what="special values, default range")


def check_thresholds(device, use_std):
    frames, stds, t = stack(21, 3, 1500, 3)
    thr = ([0.05, 0.2, -np.inf], [0.9, 0.6, np.inf])
    check_pairs(device, frames, stds if use_std else None, all_pairs(t), 32, None, thr=thr, what="thresholds")
    check_pairs(device, frames, stds if use_std else None, all_pairs(t), 32, (-0.05, 0.05), thr=thr, mask=0b011, what="thresholds, mask")
    # a channel that the thresholds remove altogether: every bin 0.0, the default range (0, 1)
    gone = ([0.0, 2.0, 0.0], [1.0, 3.0, 1.0])
    got, _ = check_pairs(device, frames, stds if use_std else None, all_pairs(t), 32, None, thr=gone, what="thresholds remove channel 1")
    assert np.all(got[:, :, 1] == 0.0)
    res = eng(device, "pairs_histogram", [T(f, device) for f in frames], [T(s, device) for s in stds] if use_std else None, all_pairs(t), 32, None,
              [1], thresholds=gone)
    for ab, rel in res:
        for h, e in (ab[1], rel[1]):
            assert np.array_equal(e, np.linspace(0.0, 1.0, 33)) and not h.any() and h.dtype == (np.float64 if use_std else np.int64)


def check_constant(device, use_std):
    """A constant difference: x = 0.5, y = 0.25, multiplier 0.5 -> a = 0.375, r = 3 everywhere: the default range is widened by +-0.5."""
    x, y = np.full((300, 3), 0.5), np.full((300, 3), 0.25)
    stds = [np.full((300, 3), 0.01), np.full((300, 3), 0.02)] if use_std else None
    check_pairs(device, [x, y], stds, [(0, 1, 0.5)], 10, None, what="constant")
    res = eng(device, "pairs_histogram", [T(x, device), T(y, device)], None if stds is None else [T(s, device) for s in stds], [(0, 1, 0.5)], 10, None,
              [0, 2])
    (ab, rel), = res
    assert sorted(ab) == [0, 2] and np.array_equal(ab[0][1], np.linspace(-0.125, 0.875, 11)) and np.array_equal(rel[2][1], np.linspace(2.5, 3.5, 11))
    assert ab[0][0].sum() > 0 and rel[2][0].sum() > 0


def check_alignment(device, use_std):
    """Frames viewed at an 8-byte offset work; a pointer that is not 8-byte aligned is HM_EALIGN with `out` untouched."""
    frames, stds, t = stack(8, 3, 257, 3)
    pairs = all_pairs(t)
    check_pairs(device, frames, stds if use_std else None, pairs, 32, (-0.05, 0.05), offset=True, what="8-byte offset")
    with backend(device):
        args = Args(device, [f.ravel() for f in frames], [x.ravel() for x in stds] if use_std else None, pairs)
    args.vp = C.cast((C.c_void_p * 3)(args.v[0].data_ptr(), args.v[1].data_ptr() + 4, args.v[2].data_ptr()), C.POINTER(C.c_void_p))
    edges = linspace_edges(np.tile([-0.05, 0.05], (3, 2, 3, 1)), 32)
    out = raw_hist(device, None, None, pairs, 3, 7, 32, edges, prefill=-3.0, expect=nat.HM_EALIGN, args=args)
    assert np.all(out == -3.0)
    assert np.isnan(raw_minmax(device, None, None, pairs, 3, expect=nat.HM_EALIGN, args=args)).all()


# ------------------------------------------------------------------------------------------------ status codes
def status_table(device):
    """-> the codes of a table of bad calls (both builds must give the same; tests/test_gpu_pairs_hist.py compares them)."""
    frames, stds, t = stack(4, 3, 40, 3, specials=False)
    pairs = all_pairs(t)
    n = frames[0].size
    codes = []
    with backend(device) as (lib, stream):
        a = Args(device, [f.ravel() for f in frames], [s.ravel() for s in stds], pairs)
        edges = T(linspace_edges(np.tile([0.0, 1.0], (3, 2, 3, 1)), 8), device)
        out = torch.full((3 * 2 * 3 * 8,), -1.0, dtype=torch.float64, device=device)
        ws = torch.empty(max(8, lib.hm_pairs_histogram_workspace_bytes(3, 8, 3) // 8), dtype=torch.float64, device=device)
        lo, hi = limits(([0.0] * 3, [1.0] * 3), 3)
        bad_pi = (C.c_int32 * 3)(0, 3, 1)
        neg_pj = (C.c_int32 * 3)(1, -1, 2)
        null_frame = C.cast((C.c_void_p * 3)(a.v[0].data_ptr(), None, a.v[2].data_ptr()), C.POINTER(C.c_void_p))
        base = dict(vals=a.vp, stds=a.sp, nf=3, pi=a.pi, pj=a.pj, pm=a.pm, P=3, n=n, C=3, mask=7, lo=lo, hi=hi, edges=edges.data_ptr(), bins=8,
                    out=out.data_ptr(), ws=ws.data_ptr())
        table = [("ok", {}, nat.HM_OK), ("vals NULL", dict(vals=None), nat.HM_EINVAL), ("pair_i NULL", dict(pi=None), nat.HM_EINVAL),
                 ("pair_j NULL", dict(pj=None), nat.HM_EINVAL), ("multipliers NULL", dict(pm=None), nat.HM_EINVAL),
                 ("out NULL", dict(out=None), nat.HM_EINVAL), ("workspace NULL", dict(ws=None), nat.HM_EINVAL),
                 ("n = 0", dict(n=0), nat.HM_EINVAL), ("n % C", dict(n=n - 1), nat.HM_EINVAL), ("C = 0", dict(C=0), nat.HM_EINVAL),
                 ("C = 5", dict(C=5, mask=1), nat.HM_EINVAL), ("no frames", dict(nf=0), nat.HM_EINVAL),
                 ("33 frames", dict(nf=33), nat.HM_EINVAL), ("no pairs", dict(P=0), nat.HM_EINVAL),
                 ("lower without upper", dict(hi=None), nat.HM_EINVAL), ("upper without lower", dict(lo=None), nat.HM_EINVAL),
                 ("a NULL frame", dict(vals=null_frame), nat.HM_EINVAL), ("pair index 3", dict(pi=bad_pi), nat.HM_EINVAL),
                 ("pair index -1", dict(pj=neg_pj), nat.HM_EINVAL), ("frames 2 of 3", dict(nf=2), nat.HM_EINVAL),
                 ("bins = 0", dict(bins=0), nat.HM_EINVAL), ("bins = 2049", dict(bins=2049), nat.HM_EINVAL),
                 ("mask bit 3", dict(mask=8), nat.HM_EINVAL), ("mask -1", dict(mask=-1), nat.HM_EINVAL), ("edges NULL", dict(edges=None), nat.HM_EINVAL),
                 ("no thresholds", dict(lo=None, hi=None), nat.HM_OK), ("no stds", dict(stds=None), nat.HM_OK), ("mask 0", dict(mask=0), nat.HM_OK)]
        hist_only = {"bins = 0", "bins = 2049", "mask bit 3", "mask -1", "edges NULL"}
        for name, change, want in table:
            k = dict(base, **change)
            out.fill_(-1.0)
            rc = lib.hm_pairs_histogram(k["vals"], k["stds"], k["nf"], k["pi"], k["pj"], k["pm"], k["P"], k["n"], k["C"], k["mask"], k["lo"], k["hi"],
                                        k["edges"], k["bins"], k["out"], k["ws"], stream)
            assert rc == want, (name, rc, want)
            if rc != nat.HM_OK:
                assert bool((out == -1.0).all()), f"{name}: out was written"
            rc2 = lib.hm_pairs_minmax(k["vals"], k["stds"], k["nf"], k["pi"], k["pj"], k["pm"], k["P"], k["n"], k["C"], k["lo"], k["hi"], k["out"],
                                      k["ws"], stream)
            assert rc2 == (nat.HM_OK if name in hist_only else want), (name, rc2)
            codes.append((name, rc, rc2))
        assert lib.hm_pairs_histogram_workspace_bytes(3, 8, 3) > 0 and lib.hm_pairs_histogram_workspace_bytes(-1, 0, 9) > 0
    return codes


# ------------------------------------------------------------------------------------------------ the Python layer
def features(t):
    return {"exposure": float(t), "subject": "linearity", "illumination": "bf", "magnification": "5x"}


def series_of(device, frames, stds, t, shape):
    cuda = sl.is_cuda(device)
    up = (lambda a: torch.tensor(a.reshape(shape), device=device)) if cuda else (lambda a: a.reshape(shape).copy())
    sets = [ImageSet(value=up(f), std=None if stds is None else up(s), features=features(ti), use_cupy=cuda)
            for f, s, ti in zip(frames, stds or [None] * len(frames), t)]
    series = ExposureSeries(input_image_sets=sets)
    series.initialize_exposure_pairs()
    return series


def per_pair_loop(series, bins, rng, channels, use_std):
    out = []
    for pair in series.exposure_pairs:
        pair.compute_difference()
        out.append(pair.process_linearity_distribution(bins, rng, channels, use_std))
        pair.absolute_difference = pair.relative_difference = None
    return out


def same_distributions(got, want, weighted, npix=24 * 17):
    """Weighted: both sides are within (k_b + 2) u sum_b |1 / std| of the exact sum, k_b <= npix, and the weights here are >= 0, so
    sum |1 / std| is the bin itself: a relative 2 (npix + 3) u."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for gd, wd in zip(g, w):
            assert sorted(gd) == sorted(wd)
            for c in gd:
                assert np.array_equal(gd[c][1], wd[c][1]) and gd[c][0].dtype == wd[c][0].dtype, c
                if weighted:
                    np.testing.assert_allclose(gd[c][0], wd[c][0], rtol=2 * (npix + 3) * U, atol=0)
                else:
                    assert np.array_equal(gd[c][0], wd[c][0])


def snapshot(series):
    m = [s.measurand for s in series.input_image_sets]
    return [(x._f64().clone(), None if x._std is None else x._std.clone()) for x in m]


def check_series(device, calls):
    """ExposureSeries.process_linearity_distribution against the per-pair loop; `calls` -> the number of hm_pairs_histogram calls so far."""
    frames, stds, t = stack(90, 4, 24 * 17, 3, ratio=1.7)
    for use_std in (False, True):
        for rng, channels in (((-0.05, 0.05), None), (None, [2, 0]), (None, [1])):
            series = series_of(device, frames, stds, t, (24, 17, 3))
            assert len(series.exposure_pairs) == 6
            before, n0 = snapshot(series), calls()
            got = series.process_linearity_distribution(48, rng, channels, use_std)
            assert calls() == n0 + 1
            for (v, s), (v0, s0) in zip(snapshot(series), before):
                assert torch.equal(v.view(torch.int64), v0.view(torch.int64)) and torch.equal(s.view(torch.int64), s0.view(torch.int64))
            same_distributions(got, per_pair_loop(series, 48, rng, channels, use_std), use_std)
    # thresholds as read: the images stay as they were; the reference is the loop over thresholded copies
    series = series_of(device, frames, stds, t, (24, 17, 3))
    lower, upper = [0.05, None, 0.1], [0.7, 0.5, None]
    before = snapshot(series)
    got = series.process_linearity_distribution(48, None, None, True, lower=lower, upper=upper)
    for (v, s), (v0, s0) in zip(snapshot(series), before):
        assert torch.equal(v.view(torch.int64), v0.view(torch.int64)) and torch.equal(s.view(torch.int64), s0.view(torch.int64))
    thresholded = series_of(device, frames, stds, t, (24, 17, 3))
    for s_ in thresholded.input_image_sets:
        s_.measurand.apply_thresholds(lower, upper)
    same_distributions(got, per_pair_loop(thresholded, 48, None, None, True), True)
    # fallbacks: one image of another shape; use_std without a std on every image; more bins than the fused path takes
    n0 = calls()
    odd = series_of(device, frames, stds, t, (24, 17, 3))
    other = series_of(device, [f[:24 * 16 * 3 // 3] for f in frames], [x[:24 * 16] for x in stds], t, (24, 16, 3))
    odd.input_image_sets[3] = other.input_image_sets[3]
    sets = odd.input_image_sets
    odd.exposure_pairs = [ExposurePair(sets[i], sets[j]) for i in range(3) for j in range(3) if i < j]
    same_distributions(odd.process_linearity_distribution(16, (-0.05, 0.05), None, True), per_pair_loop(odd, 16, (-0.05, 0.05), None, True), True)
    no_std = series_of(device, frames, None, t, (24, 17, 3))
    same_distributions(no_std.process_linearity_distribution(16, None, None, True), per_pair_loop(no_std, 16, None, None, True), False)
    many = series_of(device, frames, None, t, (24, 17, 3))
    same_distributions(many.process_linearity_distribution(2049, (-0.05, 0.05), [0], False), per_pair_loop(many, 2049, (-0.05, 0.05), [0], False), False)
    assert calls() == n0
    fused_no_std = series_of(device, frames, None, t, (24, 17, 3))
    same_distributions(fused_no_std.process_linearity_distribution(16, None, None, False), per_pair_loop(fused_no_std, 16, None, None, False), False)
    assert calls() == n0 + 1


# ------------------------------------------------------------------------------------------------ the host build
HOST = "cpu"
STD = pytest.mark.parametrize("use_std", [False, True])


@STD
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
@pytest.mark.parametrize("name,npix", SIZES)
def test_sizes(name, npix, C_, use_std):
    check_sizes(HOST, npix, C_, use_std)


@STD
def test_masks(use_std):
    check_masks(HOST, use_std)


@STD
def test_seven_frames(use_std):
    check_seven_frames(HOST, use_std)


@STD
def test_thirty_two_frames(use_std):
    check_thirty_two_frames(HOST, use_std)


@STD
@pytest.mark.parametrize("bins,C_", BINS)
def test_bins(bins, C_, use_std):
    check_bins(HOST, bins, C_, use_std)


def test_above_limit():
    check_above_limit(HOST)


@STD
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("lo,hi,bins,C_", EDGE_SETS)
def test_edges(lo, hi, bins, C_, kind, use_std):
    check_edges(HOST, lo, hi, bins, C_, kind, use_std)


def test_specials():
    check_specials(HOST)


@STD
def test_thresholds(use_std):
    check_thresholds(HOST, use_std)


@STD
def test_constant(use_std):
    check_constant(HOST, use_std)


@STD
def test_alignment(use_std):
    check_alignment(HOST, use_std)


def test_status_codes():
    status_table(HOST)


def test_series():
    check_series(HOST, lambda: nat.host_lib().calls["hm_pairs_histogram"])
