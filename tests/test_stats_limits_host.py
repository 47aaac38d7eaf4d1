"""The reductions and selection kernels beside the merge at the limits of their ABI: hm_channel_histogram / hm_channel_minmax
(csrc/hm_stats_hist.hip: k_hist, k_hist_final, k_minmax, k_minmax_final), hm_roi_mean_u8 / _f64 (csrc/hm_corrections.hip: k_roi_partial,
k_roi_final) and the standalone hm_hot_pixel_filter_u8 / _f64 (k_hot_filter, k_hot_filter_burst, wave_median, lane_median), on the
HOST build (csrc_host/hm_host.cpp), against NumPy references in extended precision written here. The checks are functions of a device
name: tests/test_gpu_stats_limits.py runs the same ones on the MI355X.

Histogram (hist_reference, check_hist)
    Reference: np.histogram on the counted values (finite; with std, std != 0), weights None or 1 / std. The bin of a value is
    np.searchsorted(edges, x, 'right') - 1 with the last edge inclusive (asserted to reproduce np.histogram's counts), and per bin
    the count k_b, sum(1 / std) and sum(|1 / std|) are formed in np.longdouble.
    Asserted: unweighted counts equal; hist.sum() equals the number of counted values in range; edges equal np.linspace(lo, hi,
    bins + 1) bit for bit; a bin the reference leaves empty is exactly 0.0; NaN / inf patterns equal; every other weighted bin obeys
        |got - ref| <= (k_b + 2) u sum_b |1 / std|,   u = 2^-53
    - one rounding for each reciprocal, k_b - 1 additions IN ANY ORDER (LDS atomics leave the device order free; the host build adds
    in index order), one for the reference's conversion. hm_channel_minmax is exact.

ROI mean (check_roi)
    Reference: img[x0:x1, y0:y1].astype(np.longdouble).sum((0, 1)), / 255 for uint8, / the pixel count.
    uint8: EXACT - every partial sum of DNs is an integer below 2^53, so any summation order gives S, and both builds then perform
    exactly (S / 255) / count in float64.
    float64: |got - ref| <= (d + 2) u sum|v| / count, d = the additions on the longest path of one value, 2 = the two divisions.
        HIP     k_roi_partial runs G = min(1024, ceil(total / 256)) workgroups of 256 lanes over total = count C elements: a lane's
                serial chain over its ceil(total / (256 G)) elements (the other channels' accumulators add exact zeros), six
                shuffle steps of wave_sum, three additions over the four waves' LDS slots; k_roi_final: one workgroup, a lane's
                chain over ceil(G / 256) partials, six shuffle steps, three LDS additions:
                d = ceil(total / (256 G)) + 9 + ceil(G / 256) + 9
        host    one running sum per channel over the ROI in row order: d = count
    Every case plants 255 (uint8) or 1e300 (float64) in every pixel OUTSIDE the ROI and keeps the inside below 255 / below 1: a read
    one row or column off breaks equality, or the bound by hundreds of orders of magnitude.

Hot-pixel filter (check_hot)
    Reference: oracle.hot_pixel_filter over oracle.median_filter_reflect (NumPy), bit for bit (np.array_equal, so -0.0 == 0.0).
    NaN frame values are out of scope: the three medians (wave-cooperative rank counting, the 19-exchange network for k = 3, per-lane
    rank counting for k = 5, 7) are not required to agree on unordered input, and the reference project's
    scipy.ndimage.median_filter gives no defined answer there.

Every check records its largest error as a fraction of its bound; the module prints the maxima at its end."""
import contextlib

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from camera_linearity_amd.measurand_factory import Measurand
from oracle import hdr_oracle as orc

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the references need an extended-precision np.longdouble (x87: 64-bit significand)"
U = 2.0 ** -53
WORST = {}                                                                  # family -> largest error / bound seen


@pytest.fixture(scope="module", autouse=True)
def report_observed_maxima():
    """After the module's tests: the largest error of each family in units of its bound (DESIGN.md section 5 quotes them)."""
    yield
    print("\nobserved maxima, in units of the bound:", {k: round(v, 4) for k, v in sorted(WORST.items())})


# ------------------------------------------------------------------------------------------------ plumbing
def is_cuda(device):
    return str(device).startswith("cuda")


def family(device, what):
    return f"{what} {'hip' if is_cuda(device) else 'host'}"


def T(a, device):
    return torch.tensor(np.ascontiguousarray(a), device=device)            # (a copy: the cases' arrays are never modified)


def M(device, v, s=None):
    return Measurand(np.array(v), None if s is None else np.array(s), use_cupy=is_cuda(device))


@contextlib.contextmanager
def backend(device):
    """-> (the library that computes on `device`, the stream argument of its entry points)."""
    if is_cuda(device):
        with torch.cuda.device(device):
            yield nat.hip_lib, nat.current_stream_ptr(torch.device(device))
    else:
        with nat.host_mode():
            yield nat.host_lib(), None


def eng(device, name, *a, **k):
    with backend(device):
        return getattr(engine, name)(*a, **k)


def offset_by_8(a, device):
    """A float64 tensor with the values of `a` whose data pointer is 8-byte but not 16-byte aligned."""
    a = np.ascontiguousarray(a, np.float64)
    big = torch.zeros(a.size + 2, dtype=torch.float64, device=device)
    k = 1 if big.data_ptr() % 16 == 0 else 0
    view = big[k:k + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


def record(fam, err, bound):
    """err, bound: arrays of equal shape (longdouble / float64), bound > 0 wherever it is used."""
    err, bound = np.asarray(err, LD), np.asarray(bound, LD)
    worst = float((err / bound).max()) if err.size else 0.0
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    return worst


# ------------------------------------------------------------------------------------------------ 1: histogram and min / max
def counted(x, s):
    keep = np.isfinite(x)
    return keep if s is None else keep & (s != 0)


def bin_index(edges, x):
    """Bin of every x in [edges[0], edges[-1]]: searchsorted, the last edge inclusive."""
    idx = np.searchsorted(edges, x, "right") - 1
    return np.where(x == edges[-1], len(edges) - 2, idx)


def hist_reference(x, s, bins, rng):
    """One channel: x (and its stds s, or None) -> dict(counts, edges, k (per bin), wsum, wabs (longdouble, None without s), inrange)."""
    keep = counted(x, s)
    xs = x[keep]
    with np.errstate(all="ignore"):
        w64 = None if s is None else 1.0 / s[keep]
        counts, edges = np.histogram(xs, bins=bins, range=rng)
    lo, hi = float(edges[0]), float(edges[-1])
    assert np.array_equal(edges, np.linspace(lo, hi, bins + 1))
    inr = (xs >= lo) & (xs <= hi)
    idx = bin_index(edges, xs[inr])
    k = np.bincount(idx, minlength=bins)
    assert np.array_equal(k, counts), "searchsorted does not reproduce np.histogram"
    ref = dict(counts=counts, edges=edges, k=k, wsum=None, wabs=None, inrange=int(inr.sum()))
    if s is not None:
        with np.errstate(all="ignore"):
            w = np.where(np.isfinite(w64), LD(1) / s[keep].astype(LD), w64.astype(LD))[inr]      # float64's inf / 0 weights stay what they are
            ref["wsum"], ref["wabs"] = np.zeros(bins, LD), np.zeros(bins, LD)
            np.add.at(ref["wsum"], idx, w)
            np.add.at(ref["wabs"], idx, np.abs(w))
    return ref


def assert_hist(fam, got_h, got_e, ref, weighted, what):
    assert np.array_equal(got_e, ref["edges"]), f"{what}: edges"
    got_h = np.asarray(got_h)
    assert got_h.shape == ref["counts"].shape, what
    if not weighted:
        assert np.array_equal(got_h, ref["counts"]), f"{what}: counts differ in {np.flatnonzero(got_h != ref['counts'])[:8]}"
        assert int(got_h.sum()) == ref["inrange"], what
        return 0.0
    got_h = got_h.astype(np.float64)
    wsum, wabs, k = ref["wsum"], ref["wabs"], ref["k"]
    assert np.all(got_h[k == 0] == 0.0), f"{what}: a bin the reference leaves empty is not 0.0"
    np.testing.assert_array_equal(np.isnan(got_h), np.isnan(wsum), err_msg=f"{what}: NaN pattern")
    np.testing.assert_array_equal(np.isposinf(got_h), np.isposinf(wsum), err_msg=f"{what}: +inf pattern")
    np.testing.assert_array_equal(np.isneginf(got_h), np.isneginf(wsum), err_msg=f"{what}: -inf pattern")
    fin = np.isfinite(wsum) & (k > 0) & np.isfinite(wabs) & (wabs > 0)
    assert np.all(got_h[np.isfinite(wsum) & (k > 0) & (wabs == 0)] == 0.0), what                 # (only zero weights: std = inf)
    if not fin.any():
        return 0.0
    worst = record(fam, np.abs(got_h[fin].astype(LD) - wsum[fin]), (k[fin] + 2) * LD(U) * wabs[fin])
    assert worst <= 1.0, f"{what}: {worst:.3f} x the bound (k_b + 2) u sum|1/std|"
    return worst


def check_hist(device, v, s, bins, rng, channels=None, use_std=False, what="histogram"):
    """v, s: (..., C) arrays. Through Measurand.compute_channel_histogram; every requested channel against hist_reference."""
    C_ = v.shape[-1]
    channels = list(range(C_)) if channels is None else channels
    got = M(device, v, s).compute_channel_histogram(bins, rng, channels, use_std)
    assert sorted(got) == sorted(channels)
    for c in channels:
        ref = hist_reference(v[..., c].ravel(), s[..., c].ravel() if use_std else None, bins, rng)
        assert_hist(family(device, "histogram"), got[c][0], got[c][1], ref, use_std, f"{what}, channel {c}")
    return got


def raw_minmax(device, flat_v, flat_s, C_):
    with backend(device) as (lib, stream):
        v = T(flat_v, device)
        s = None if flat_s is None else T(flat_s, device)
        out = torch.full((2 * C_,), float("nan"), dtype=torch.float64, device=device)
        ws = torch.empty(max(8, lib.hm_histogram_workspace_bytes(1, C_) // 8), dtype=torch.float64, device=device)
        rc = lib.hm_channel_minmax(v.data_ptr(), nat.ptr(s), v.numel(), C_, out.data_ptr(), ws.data_ptr(), stream)
        assert rc == nat.HM_OK
        return out.cpu().numpy().reshape(C_, 2)


def raw_hist(device, flat_v, flat_s, C_, mask, bins, lo, hi, prefill=float("nan"), expect=nat.HM_OK):
    """hm_channel_histogram called directly -> out (C, bins) (pre-filled with `prefill`), or None when `expect` is an error code."""
    with backend(device) as (lib, stream):
        v = T(flat_v, device)
        s = None if flat_s is None else T(flat_s, device)
        edges = T(np.linspace(lo, hi, bins + 1), device)
        out = torch.full((C_ * bins,), prefill, dtype=torch.float64, device=device)
        ws = torch.empty(max(8, lib.hm_histogram_workspace_bytes(bins, C_) // 8), dtype=torch.float64, device=device)
        rc = lib.hm_channel_histogram(v.data_ptr(), nat.ptr(s), v.numel(), C_, mask, edges.data_ptr(), bins, lo, hi, out.data_ptr(),
                                      ws.data_ptr(), stream)
        assert rc == expect, (rc, expect)
        return out.cpu().numpy().reshape(C_, bins) if rc == nat.HM_OK else None


def check_minmax(device, flat_v, flat_s, C_):
    got = raw_minmax(device, flat_v, flat_s, C_)
    for c in range(C_):
        x, s = flat_v[c::C_], None if flat_s is None else flat_s[c::C_]
        xs = x[counted(x, s)]
        ref = (xs.min(), xs.max()) if xs.size else (np.inf, -np.inf)
        assert got[c, 0] == ref[0] and got[c, 1] == ref[1], (c, got[c], ref)
    return got


def flat_data(seed, n, nan_ends=True):
    """n values in [0, 1) with NaNs, infinities, values on the range ends 0.1 / 0.9 and outside them; stds with zeros."""
    rng = np.random.default_rng(seed)
    v = rng.random(n)
    s = 0.05 + rng.random(n)
    m = max(1, n // 50)
    for val in (np.nan, np.inf, -np.inf, 0.1, 0.9, -0.25, 1.5):
        v[rng.integers(0, n, m)] = val
    s[rng.integers(0, n, m)] = 0.0
    if nan_ends:
        v[0] = v[-1] = np.nan                                               # the first value of the array NaN, and the last
    return v, s


HIST_COUNTS = [200, 65536, 3 * 43713]        # less than one workgroup; the grid of 256 x 256 lanes exactly full; three trips, the last ragged


def check_hist_counts(device, C_, n, use_std):
    """The raw ABI on n elements (channel = index % C; n need not be a multiple of C): every channel, and the min / max."""
    v, s = flat_data(1000 * C_ + n % 997, n)
    s = s if use_std else None
    lo, hi, bins = 0.1, 0.9, 32
    got = raw_hist(device, v, s, C_, (1 << C_) - 1, bins, lo, hi)
    for c in range(C_):
        ref = hist_reference(v[c::C_], None if s is None else s[c::C_], bins, (lo, hi))
        assert_hist(family(device, "histogram"), got[c] if use_std else got[c].astype(np.int64), ref["edges"], ref, use_std,
                    f"C={C_} n={n} channel {c}")
    check_minmax(device, v, s, C_)


HIST_BINS = [(1, 3), (2, 3), (255, 3), (256, 3), (257, 3), (2048, 4), (8192, 1)]      # (bins, C): the LDS loops make one, one-and-a-bit, many trips


def check_hist_bins(device, bins, C_, use_std):
    n = 20000 if bins > 1000 else 2999
    v, s = flat_data(bins + C_, n * C_)
    check_hist(device, v.reshape(n, C_), s.reshape(n, C_), bins, (0.1, 0.9), None, use_std, f"bins={bins} C={C_}")


def check_hist_above_limit(device):
    """bins * C = 8193: NotImplementedError from the Measurand, HM_EUNSUPPORTED from the entry point of either build."""
    v = np.linspace(0, 1, 24)
    for bins, C_ in ((8193, 1), (2731, 3)):
        with pytest.raises(NotImplementedError):
            M(device, v.reshape(-1, C_)).compute_channel_histogram(bins, (0.0, 1.0), list(range(C_)), False)
        raw_hist(device, v, None, C_, (1 << C_) - 1, bins, 0.0, 1.0, expect=nat.HM_EUNSUPPORTED)
    assert raw_hist(device, v, None, 1, 1, 8192, 0.0, 1.0) is not None


EDGE_SETS = [(0.1, 0.9, 32, 3, 9), (0.0, 1.0, 255, 3, 24), (-0.3, 0.7, 257, 3, 135), (0.1, 0.9, 2048, 4, 583), (1e-3, 3e-3, 8192, 1, 2293)]


def edge_inputs(lo, hi, bins):
    """Every edge, its np.nextafter below (except the first edge) and above (except the last)."""
    e = np.linspace(lo, hi, bins + 1)
    return np.concatenate([e, np.nextafter(e[1:], -np.inf), np.nextafter(e[:-1], np.inf)])


def uncorrected_differs(lo, hi, bins):
    """NumPy alone: on how many edge inputs below the last edge the index int((x - lo) * (bins / (hi - lo))) misses the reference bin
    -> (count, inputs, max |miss| over all inputs, the uncorrected index of the last edge)."""
    x = edge_inputs(lo, hi, bins)
    raw = ((x - lo) * (bins / (hi - lo))).astype(np.int64)
    ref = bin_index(np.linspace(lo, hi, bins + 1), x)
    miss = np.abs(raw - ref)
    return int((miss[x != hi] != 0).sum()), x.size, int(miss.max()), int(raw[x == hi][0])


@pytest.mark.parametrize("lo,hi,bins,C_,differ", EDGE_SETS)
def test_edge_inputs_need_every_correction(lo, hi, bins, C_, differ):
    """The precondition of the edge-value cases: the uncorrected index is wrong for `differ` inputs of the set (the comparisons with
    edges[idx] and edges[idx + 1] put them right) and is `bins` for the last edge (the `idx == bins` step), never off by more than 1 -
    so a kernel that lost one of the corrections fails these cases."""
    count, total, worst, last = uncorrected_differs(lo, hi, bins)
    print(f"\n({lo}, {hi}, {bins}): {count} of {total} edge inputs differ, by at most {worst}")
    assert total == 3 * (bins + 1) - 2 and count >= 1 and worst == 1 and last == bins
    assert count == differ


def check_hist_edges(device, lo, hi, bins, C_, use_std):
    rng = np.random.default_rng(bins)
    x = np.concatenate([edge_inputs(lo, hi, bins), [lo - 1.0, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), hi + 1.0, hi, hi]])
    x = np.concatenate([x, rng.choice(x, (-x.size) % C_)])                  # fill the last pixel
    rng.shuffle(x)
    v = x.reshape(-1, C_)
    s = 0.05 + rng.random(v.shape)
    check_hist(device, v, s, bins, (lo, hi), None, use_std, f"edge values ({lo}, {hi}, {bins})")


def subset_data():
    """(1500, 3): channels 0 and 1 span exactly [0.2, 0.8], channel 2 spans [-3, 5]."""
    rng = np.random.default_rng(77)
    v = 0.2 + 0.6 * rng.random((1500, 3))
    v[:, 2] = -3 + 8 * rng.random(1500)
    v[3, 0], v[9, 0], v[5, 1], v[7, 1], v[2, 2], v[4, 2] = 0.2, 0.8, 0.2, 0.8, -3.0, 5.0
    v[11, 1] = np.nan
    return v, 0.05 + rng.random(v.shape)


def check_hist_subsets(device, use_std):
    """included_range=None: one launch per distinct range; a proper subset of channels; channels in another order."""
    v, s = subset_data()
    with backend(device) as (lib, _):
        pass
    for channels, launches in (([1], 1), ([2, 0], 2), ([0, 1], 1), ([0, 1, 2], 2)):
        before = lib.calls["hm_channel_histogram"]
        got = check_hist(device, v, s, 64, None, channels, use_std, f"channels={channels}")
        assert lib.calls["hm_channel_histogram"] == before + launches
        assert list(got) == channels or sorted(got) == sorted(channels)


def check_hist_unmasked(device, use_std):
    """Raw ABI, out pre-filled with NaN, channel_mask 0b0101 of C = 4: channels 1 and 3 come back as 0.0."""
    v, s = flat_data(5, 4 * 700)
    s = s if use_std else None
    got = raw_hist(device, v, s, 4, 0b0101, 48, 0.1, 0.9)
    assert np.all(got[1] == 0.0) and np.all(got[3] == 0.0)
    for c in (0, 2):
        ref = hist_reference(v[c::4], None if s is None else s[c::4], 48, (0.1, 0.9))
        assert_hist(family(device, "histogram"), got[c] if use_std else got[c].astype(np.int64), ref["edges"], ref, use_std, f"mask, channel {c}")


def empty_data():
    """(300, 4): channel 0 all NaN, channel 1 ordinary values whose stds are all zero, channel 2 +-inf only, channel 3 ordinary."""
    rng = np.random.default_rng(91)
    v = rng.random((300, 4))
    s = 0.05 + rng.random((300, 4))
    v[:, 0] = np.nan
    s[:, 1] = 0.0
    v[:, 2] = np.where(rng.random(300) < 0.5, np.inf, -np.inf)
    return v, s


def check_hist_nothing_to_count(device, use_std):
    """np.histogram of an empty selection: zero counts on np.linspace(0, 1, bins + 1). The other channels are unaffected."""
    v, s = empty_data()
    bins = 16
    got = check_hist(device, v, s, bins, None, None, use_std, "nothing to count")
    for c in (0, 2) + ((1,) if use_std else ()):
        assert np.array_equal(got[c][1], np.linspace(0, 1, bins + 1)) and not np.any(got[c][0]) and len(got[c][0]) == bins
    assert got[3][0].sum() > 0 and (use_std or got[1][0].sum() == 300)
    mm = check_minmax(device, v.ravel(), s.ravel() if use_std else None, 4)
    assert np.array_equal(mm[0], [np.inf, -np.inf]) and np.array_equal(mm[2], [np.inf, -np.inf])
    check_hist(device, v[:, :1], s[:, :1], bins, None, [0], use_std, "one channel, all NaN")


def check_hist_constant(device, use_std):
    """A constant channel with included_range=None: np.histogram widens the range by +-0.5."""
    rng = np.random.default_rng(17)
    v = rng.random((400, 3))
    v[:, 1] = 0.25
    v[::7, 1] = np.nan
    for bins in (1, 10, 33):
        got = check_hist(device, v, 0.05 + rng.random(v.shape), bins, None, None, use_std, f"constant channel, bins={bins}")
        assert got[1][1][0] == -0.25 and got[1][1][-1] == 0.75


def check_hist_special_stds(device):
    """A negative std is a negative weight, 5e-324 the weight +inf, inf the weight 0."""
    rng = np.random.default_rng(23)
    v = rng.random((900, 3))
    s = 0.05 + rng.random(v.shape)
    s[rng.random(v.shape) < 0.2] *= -1.0
    v[:, 1] = 0.1 + 0.8 * (np.arange(900) % 8 + 0.5) / 8                   # channel 1: eight bins, special stds in known ones
    s[v[:, 1] < 0.2, 1] = np.inf                                            # bin 0: weights 0 only
    s[np.flatnonzero((v[:, 1] > 0.2) & (v[:, 1] < 0.3))[:3], 1] = 5e-324    # bin 1: +inf
    i2 = np.flatnonzero((v[:, 1] > 0.3) & (v[:, 1] < 0.4))
    s[i2[0], 1], s[i2[1], 1] = 5e-324, -5e-324                              # bin 2: +inf and -inf -> NaN
    s[np.flatnonzero((v[:, 1] > 0.4) & (v[:, 1] < 0.5))[:2], 1] = -5e-324   # bin 3: -inf
    got = check_hist(device, v, s, 8, (0.1, 0.9), None, True, "special stds")
    h = got[1][0]
    assert h[0] == 0.0 and np.isposinf(h[1]) and np.isnan(h[2]) and np.isneginf(h[3]) and np.all(np.isfinite(h[4:]))


def check_hist_nan_ends(device, use_std):
    v, s = flat_data(3, 3 * 501)
    assert np.isnan(v[0]) and np.isnan(v[-1])
    check_hist(device, v.reshape(-1, 3), s.reshape(-1, 3), 20, None, None, use_std, "NaN first and last")


def check_hist_offset_view(device, use_std):
    """engine.channel_histogram on float64 views that are only 8-byte aligned (values and stds)."""
    v, s = flat_data(4, 3 * 777)
    v, s = v.reshape(-1, 3), s.reshape(-1, 3)
    vt, st = offset_by_8(v, device), offset_by_8(s, device) if use_std else None
    for rng in (None, (0.1, 0.9)):
        got = eng(device, "channel_histogram", vt, st, 40, rng, [0, 1, 2])
        for c in range(3):
            ref = hist_reference(v[:, c], s[:, c] if use_std else None, 40, rng)
            assert_hist(family(device, "histogram"), got[c][0], got[c][1], ref, use_std, f"offset view, channel {c}")
    check_minmax(device, v.ravel(), s.ravel() if use_std else None, 3)


# ------------------------------------------------------------------------------------------------ 2: ROI mean
def roi_depth(device, count, C_):
    """Additions on the longest path of one value through the implementation (module docstring)."""
    if not is_cuda(device):
        return count
    total = count * C_
    G = min(1024, -(-total // 256))
    return -(-total // (256 * G)) + 9 + -(-G // 256) + 9


def test_roi_depth_counts():
    assert roi_depth("cuda:0", 1, 1) == 1 + 9 + 1 + 9 and roi_depth("cuda:0", 300 * 300, 3) == 2 + 9 + 4 + 9
    assert roi_depth("cuda:0", 40 * 50, 4) == 1 + 9 + 1 + 9 and roi_depth("cpu", 40 * 50, 4) == 2000


def planted_image(seed, H, W, C_, roi, f64):
    """Inside the ROI values below 255 / below 1, everywhere else 255 / 1e300."""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = roi
    if f64:
        img = np.full((H, W, C_), 1e300)
        img[x0:x1, y0:y1] = rng.random((x1 - x0, y1 - y0, C_))
    else:
        img = np.full((H, W, C_), 255, np.uint8)
        img[x0:x1, y0:y1] = rng.integers(0, 255, (x1 - x0, y1 - y0, C_))
    return img


def check_roi(device, img, roi, tensor=None, what="roi"):
    x0, x1, y0, y1 = roi
    C_ = img.shape[-1]
    count = (x1 - x0) * (y1 - y0)
    got = eng(device, "roi_mean", T(img, device) if tensor is None else tensor, x0, x1, y0, y1).cpu().numpy()
    sel = img[x0:x1, y0:y1]
    assert got.shape == (C_,)
    if img.dtype == np.uint8:
        S = sel.astype(np.int64).sum((0, 1))
        expect = (S.astype(np.float64) / 255.0) / count
        assert np.array_equal(got, expect), f"{what} {roi}: {got} != {expect}"
        ref = sel.astype(LD).sum((0, 1)) / LD(255) / LD(count)
        assert np.all(np.abs(got.astype(LD) - ref) <= 2 * U * ref)
        return
    ref = sel.astype(LD).sum((0, 1)) / LD(count)
    bound = (roi_depth(device, count, C_) + 2) * LD(U) * np.abs(sel).astype(LD).sum((0, 1)) / LD(count)
    worst = record(family(device, "roi mean f64"), np.abs(got.astype(LD) - ref), bound)
    assert worst <= 1.0, f"{what} {roi}: {worst:.3g} x the bound"


def small_rois(H, W):
    return [(0, H, 0, W), (0, 1, 0, 1), (H - 1, H, W - 1, W), (7, 8, 0, W), (0, H, 11, 12), (3, 17, 5, 6), (3, 4, 5, 31)]


def check_roi_small(device, C_, f64):
    H, W = 40, 50
    for i, roi in enumerate(small_rois(H, W)):
        check_roi(device, planted_image(10 * C_ + i, H, W, C_, roi, f64), roi)


def check_roi_large(device, f64):
    """310 x 300 x 3: 270 000 ROI elements are two trips of the 1024 x 256 grid, the second ragged; 195 are less than a workgroup."""
    for i, roi in enumerate([(5, 305, 0, 300), (100, 105, 7, 20)]):
        check_roi(device, planted_image(50 + i, 310, 300, 3, roi, f64), roi)


def check_roi_offset_view(device):
    for C_ in (1, 3):
        roi = (2, 9, 1, 12)
        img = planted_image(60 + C_, 11, 13, C_, roi, True)
        check_roi(device, img, roi, tensor=offset_by_8(img, device), what="offset view")


def check_roi_status(device):
    with backend(device) as (lib, stream):
        H, W = 6, 7
        ws = torch.zeros(max(8, lib.hm_roi_mean_workspace_bytes() // 8), dtype=torch.float64, device=device)
        out = torch.zeros(8, dtype=torch.float64, device=device)
        for fn, dt in ((lib.hm_roi_mean_u8, torch.uint8), (lib.hm_roi_mean_f64, torch.float64)):
            img = torch.zeros(H * W * 5, dtype=dt, device=device)
            call = lambda C_, *roi: fn(img.data_ptr(), H, W, C_, *roi, out.data_ptr(), ws.data_ptr(), stream)   # noqa: E731
            for roi in ((0, H + 1, 0, W), (0, H, 0, W + 1), (-1, H, 0, W), (3, 3, 0, W), (0, H, 4, 3)):
                assert call(3, *roi) == nat.HM_ESHAPE, roi
            assert call(5, 0, H, 0, W) == nat.HM_EINVAL and call(0, 0, H, 0, W) == nat.HM_EINVAL
            assert call(4, 0, H, 0, W) == nat.HM_OK


# ------------------------------------------------------------------------------------------------ 3: standalone hot-pixel filter
def check_hot(device, x, dmap, k, min_dn=100, thr=0.3, hot=None, tensor=None, what="hot filter"):
    """x uint8 or float64 (H, W, C); dmap uint8 (hot iff >= min_dn) or float64 (hot iff > thr). `hot` overrides the reference's mask
    (a case that states the expected mask itself). -> (out, hot)."""
    if hot is None:
        hot = dmap >= min_dn if dmap.dtype == np.uint8 else dmap > thr
    ref = orc.hot_pixel_filter(x.astype(np.float64), hot.astype(np.float64), 0.5, k)
    out = eng(device, "hot_pixel_filter", T(x, device) if tensor is None else tensor, T(dmap, device), thr, k, min_dn).cpu().numpy()
    assert out.dtype == x.dtype and out.shape == x.shape
    bad = np.argwhere(out.astype(np.float64) != ref)
    assert bad.size == 0, f"{what} k={k} {x.shape} {x.dtype}/{dmap.dtype}: {len(bad)} elements differ, first at {bad[:4].tolist()}"
    assert np.array_equal(out[~hot], x[~hot])
    return out, hot


def hot_mask(rng, shape, density=0.02):
    """Hot on all four borders (so the four corners) and the last element, `density` elsewhere."""
    hot = rng.random(shape) < density
    hot[0], hot[-1], hot[:, 0], hot[:, -1] = True, True, True, True
    assert hot[-1, -1, -1] and hot[0, 0, 0] and not hot.all()
    return hot


def maps_of(rng, hot, min_dn=100, thr=0.3):
    u8 = np.where(hot, rng.integers(min_dn, 256, hot.shape), rng.integers(0, min_dn, hot.shape)).astype(np.uint8)
    f64 = np.where(hot, thr + 0.01 + rng.random(hot.shape), thr * rng.random(hot.shape))
    return u8, f64


HOT_SHAPES = {np.uint8: (64, 65), np.float64: (17, 33)}      # x C: whole burst spans (4096 uint8 / 512 float64 elements) and a ragged rest


def check_hot_spans(device, k, C_):
    rng = np.random.default_rng(100 * k + C_)
    for dt, (H, W) in HOT_SHAPES.items():
        span = 4096 if dt == np.uint8 else 512
        assert H * W * C_ // span >= 1 and H * W * C_ % span != 0
        x = rng.integers(0, 256, (H, W, C_)).astype(np.uint8) if dt == np.uint8 else rng.random((H, W, C_))
        hot = hot_mask(rng, x.shape)
        assert hot.reshape(-1)[:span].any() and hot.reshape(-1)[(x.size // span) * span:].any()     # hot elements in both parts
        for dmap in maps_of(rng, hot):
            out, h = check_hot(device, x, dmap, k)
            assert np.array_equal(h, hot)


THIN_SHAPES = [(1, 1, 3), (1, 9, 3), (9, 1, 3), (2, 3, 3), (3, 2, 1)]      # thinner than the median radius: reflect folds more than once


def check_hot_thin(device, shape, k):
    rng = np.random.default_rng(sum(shape) + k)
    hot = np.ones(shape, bool)
    for x in (rng.integers(0, 256, shape).astype(np.uint8), rng.random(shape)):
        for dmap in maps_of(rng, hot):
            check_hot(device, x, dmap, k)


def check_hot_thresholds(device):
    """A comparison exactly on its threshold: map_u8 >= min_dn, map_f64 > thr; min_dn = 256 nothing, min_dn = 1 all but zeros."""
    rng = np.random.default_rng(5)
    for dt, (H, W) in HOT_SHAPES.items():
        shape = (H, W, 3)
        x = rng.integers(0, 256, shape).astype(np.uint8) if dt == np.uint8 else rng.random(shape)
        m = rng.choice(np.array([99, 100, 101], np.uint8), shape)
        out, _ = check_hot(device, x, m, 3, min_dn=100, hot=(m == 100) | (m == 101), what="min_dn on the threshold")
        assert (out != x).sum() > 0.4 * x.size                              # (two thirds are hot; a median rarely equals its centre)
        m = rng.integers(0, 256, shape).astype(np.uint8)
        m[0, 0, 0], m[1, 1, 1] = 255, 0
        out, _ = check_hot(device, x, m, 3, min_dn=256, hot=np.zeros(shape, bool), what="min_dn = 256")
        assert np.array_equal(out, x)
        check_hot(device, x, m, 3, min_dn=1, hot=m != 0, what="min_dn = 1")
        thr = 0.3
        vals = np.array([np.nextafter(thr, 0), thr, np.nextafter(thr, 1)])
        mf = rng.choice(vals, shape)
        check_hot(device, x, mf, 3, thr=thr, hot=mf == vals[2], what="thr on the threshold")


def check_hot_ties(device, k):
    """Two-valued data, every element hot: the rank-counting medians break ties as the sorted window's middle element does."""
    rng = np.random.default_rng(40 + k)
    for dt, (H, W) in HOT_SHAPES.items():
        shape = (H, W, 3)
        if dt == np.uint8:
            x = rng.choice(np.array([0, 255], np.uint8), shape)
        else:
            x = rng.choice(np.array([0.25, 0.75, np.inf, -0.0, 0.0]), shape)
        hot = np.ones(shape, bool)
        for dmap in maps_of(rng, hot):
            check_hot(device, x, dmap, k, what="ties")


def check_hot_unaligned_k7(device):
    """uint8 data whose pointer is not 16-byte aligned, k = 7: everything through the wave-cooperative median at 49 lanes."""
    rng = np.random.default_rng(7)
    shape = (33, 40, 3)
    x = rng.integers(0, 256, shape).astype(np.uint8)
    hot = hot_mask(rng, shape, 0.05)
    big = torch.zeros(x.size + 16, dtype=torch.uint8, device=device)
    off = 3 if big.data_ptr() % 16 == 0 else 0
    view = big[off:off + x.size].view(shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 != 0
    check_hot(device, x, maps_of(rng, hot)[0], 7, tensor=view, what="unaligned")


# ------------------------------------------------------------------------------------------------ the host build
HOST = "cpu"
STD = pytest.mark.parametrize("use_std", [False, True])


@STD
@pytest.mark.parametrize("n", HIST_COUNTS)
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_hist_counts(C_, n, use_std):
    check_hist_counts(HOST, C_, n, use_std)


@STD
@pytest.mark.parametrize("bins,C_", HIST_BINS)
def test_hist_bins(bins, C_, use_std):
    check_hist_bins(HOST, bins, C_, use_std)


def test_hist_above_limit():
    check_hist_above_limit(HOST)


@STD
@pytest.mark.parametrize("lo,hi,bins,C_,differ", EDGE_SETS)
def test_hist_edges(lo, hi, bins, C_, differ, use_std):
    check_hist_edges(HOST, lo, hi, bins, C_, use_std)


@STD
def test_hist_subsets(use_std):
    check_hist_subsets(HOST, use_std)


@STD
def test_hist_unmasked(use_std):
    check_hist_unmasked(HOST, use_std)


@STD
def test_hist_nothing_to_count(use_std):
    check_hist_nothing_to_count(HOST, use_std)


@STD
def test_hist_constant(use_std):
    check_hist_constant(HOST, use_std)


def test_hist_special_stds():
    check_hist_special_stds(HOST)


@STD
def test_hist_nan_ends(use_std):
    check_hist_nan_ends(HOST, use_std)


@STD
def test_hist_offset_view(use_std):
    check_hist_offset_view(HOST, use_std)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_roi_small(C_, f64):
    check_roi_small(HOST, C_, f64)


@pytest.mark.parametrize("f64", [False, True])
def test_roi_large(f64):
    check_roi_large(HOST, f64)


def test_roi_offset_view():
    check_roi_offset_view(HOST)


def test_roi_status():
    check_roi_status(HOST)


@pytest.mark.parametrize("C_", [1, 2, 4])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_hot_spans(k, C_):
    check_hot_spans(HOST, k, C_)


@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("shape", THIN_SHAPES)
def test_hot_thin(shape, k):
    check_hot_thin(HOST, shape, k)


def test_hot_thresholds():
    check_hot_thresholds(HOST)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_hot_ties(k):
    check_hot_ties(HOST, k)


def test_hot_unaligned_k7():
    check_hot_unaligned_k7(HOST)
