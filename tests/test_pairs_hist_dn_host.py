"""hm_pairs_minmax_dn / hm_pairs_histogram_dn / engine.pairs_histogram_dn / ExposureSeries.process_linearity_distribution(from_dn=True): the
all-pairs linearity distributions straight from uint8 and uint16 DN frames, on the HOST build (csrc_host/hm_host.cpp). The checks are
functions of a device name: tests/test_gpu_pairs_hist_dn.py runs the same ones on the MI355X (csrc/hm_stats_hist_dn.hip: k_pairs_hist_dn,
k_pairs_minmax_dn; csrc/hm_stats_dn.hip: k_pairs_dn_table).

Oracle, two parts for every case
    1. NumPy on table-mapped values: v = icrf[DN & (2^b - 1), c], s = icrf_diff[idx, c] * std_table[idx, c] (one float64 rounding: the bits
       hm_linearize_* writes), then diff_reference / hist_reference / assert_hist of tests/test_pairs_hist_host.py per (pair, kind, channel).
    2. The route the entries replace, on the same build and device: engine.linearize of every frame (with stds: of the STD table first),
       then hm_pairs_minmax / hm_pairs_histogram on those float64 frames with the same thresholds and edges.
Asserted
    Min / max bit-equal to both parts; edges built from them bit-equal; unweighted histograms torch.equal to part 2's and equal to part 1's
    counts, their sum the in-range count; empty bins exactly 0.0; NaN / inf patterns equal; weighted bins within assert_hist's bound
    (k_b + 2) u sum_b |1 / std| of part 1 and within twice that of part 2 (each side is within the bound of the exact sum; the weights are
    the same float64 bits on both sides, because the table's product is hm_linearize_*'s single multiplication). The DN frames are
    byte-identical after every call.
Sizes and placements that come from the kernels' constants (csrc/hm_pairs_rules.h, re-derived in plan_of below)
    per_pair = 2 C bins 8 bytes, T = (8 | 16) 2^b C bytes; a launch takes min(HM_PAIRS_MAX, (160 KiB - (table in LDS ? T : 0)) / per_pair)
    pairs, the launches of equal size; variant 0 puts the table in LDS only where the call needs no more launches with it and a CU holds
    as many workgroups of the launch with it. SIZES, SPLIT_BINS: tests/test_pairs_hist_host.py.

Every check records its largest error as a fraction of its bound; the module prints the maxima at its end."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from camera_linearity_amd import settings as gs

import test_pairs_hist_host as ph
import test_pairs_stats_dn_host as dn
from test_pairs_hist_host import SIZES, FULL_SWEEP, RAGGED, SPLIT_BINS, EDGE_SETS, diff_reference, default_range, linspace_edges
from test_stats_limits_host import LD, U, backend, family, record, hist_reference, assert_hist, counted, is_cuda
from test_stats_limits_host import report_observed_maxima  # noqa: F401  (prints the observed maxima after this module too)

SYMBOLS = ("hm_pairs_histogram_dn_workspace_bytes", "hm_pairs_minmax_dn", "hm_pairs_histogram_dn", "hm_pairs_histogram_dn_describe")
LDS_BYTES = 160 * 1024
PER_CU_MAX, WAVES_PER_CU = 4, 32
BINS = (1, 256, 257, SPLIT_BINS, 2048)


# ------------------------------------------------------------------------------------------------ the fit rule, from the constants
def table_bytes(bits, C_, with_std):
    return (16 if with_std else 8) * 2 ** bits * C_


def per_cu(np_, lds):
    wpp = nat.HM_PAIRS_MAX // np_
    return max(1, min(LDS_BYTES // lds, WAVES_PER_CU // (np_ * wpp), PER_CU_MAX))


def plan_of(n_pairs, bins, C_, bits, with_std, variant):
    """-> [(pairs, waves per pair, 'lds' | 'global')] per launch, or None where variant 1 is refused."""
    per_pair, tb = 2 * C_ * bins * 8, table_bytes(bits, C_, with_std)
    ppl0 = min(nat.HM_PAIRS_MAX, LDS_BYTES // per_pair)
    ppl_t = min(nat.HM_PAIRS_MAX, max(0, LDS_BYTES - tb) // per_pair)
    launches = lambda ppl: -(-n_pairs // ppl)                                # noqa: E731
    if variant == 1:
        if ppl_t < 1:
            return None
        ppl, allowed = ppl_t, True
    else:
        ppl, allowed = ppl0, variant == 0 and ppl_t >= 1 and launches(ppl_t) == launches(ppl0)
    per = -(-n_pairs // launches(ppl))
    out = []
    for p0 in range(0, n_pairs, per):
        np_ = min(per, n_pairs - p0)
        hist = np_ * per_pair
        lds = variant == 1 or (allowed and hist + tb <= LDS_BYTES and per_cu(np_, hist + tb) == per_cu(np_, hist))
        out.append((np_, nat.HM_PAIRS_MAX // np_, "lds" if lds else "global"))
    return out


def describe_of(n_pairs, bins, C_, bits, with_std, variant):
    return " + ".join(f"pairs_hist_dn<dn={'u8' if bits == 8 else 'u16'},bits={bits},tab={tab},std={int(with_std)},np={np_},wpp={wpp}>"
                      for np_, wpp, tab in plan_of(n_pairs, bins, C_, bits, with_std, variant))


def describe(lib, n, nf, npairs, C_, with_std, bits, bins, variant):
    buf = C.create_string_buffer(1024)
    rc = lib.hm_pairs_histogram_dn_describe(n, nf, npairs, C_, int(with_std), bits, bins, variant, buf, len(buf))
    return rc, buf.value.decode()


def test_fit_rule():
    """The placements the issue names, from the constants alone."""
    assert plan_of(1, 2048, 4, 8, True, 0) == [(1, 16, "lds")] and plan_of(1, 2048, 4, 8, True, 1) == [(1, 16, "lds")]      # 128 + 16 KiB
    assert plan_of(1, 2048, 4, 12, False, 1) is None and plan_of(1, 2048, 4, 12, True, 1) is None                            # 128 + 128 KiB
    assert plan_of(1, 2048, 4, 12, False, 0) == [(1, 16, "global")]
    assert plan_of(15, 256, 3, 8, True, 0) == [(8, 2, "lds"), (7, 2, "lds")]                    # 96 / 84 + 12 KiB: one workgroup per CU either way
    assert plan_of(15, 64, 3, 8, True, 0) == [(15, 1, "lds")]                                   # 45 + 12 KiB: two workgroups (15 waves each) either way
    assert plan_of(15, 100, 3, 8, True, 0) == [(15, 1, "global")]                               # 72 000 bytes: 2 per CU without the table, 1 with it
    assert plan_of(15, 100, 3, 8, True, 1) == [(15, 1, "lds")]
    assert plan_of(15, 256, 3, 12, True, 0) == [(8, 2, "global"), (7, 2, "global")]             # T = 192 KiB
    assert plan_of(15, 256, 3, 12, False, 1) == [(5, 3, "lds")] * 3                             # T = 96 KiB leaves 64 KiB: 5 pairs
    assert plan_of(16, 1, 1, 16, False, 2) == [(16, 1, "global")]


@pytest.mark.parametrize("lib", ["host", "device"])
def test_describe(lib):
    """hm_pairs_histogram_dn_describe: the device build names the kernel of every launch as plan_of derives it; the host build a host
    name; both the same statuses. Nothing is launched (no GPU needed)."""
    if lib == "host":
        with nat.host_mode():
            L = nat.host_lib()
    else:
        L = nat.hip_lib
    for n_pairs, bins, C_, bits, with_std in ((1, 2048, 4, 8, True), (15, 256, 3, 8, True), (15, 64, 3, 8, False), (15, 256, 3, 12, True),
                                              (15, 256, 3, 12, False), (16, 256, 3, 10, True), (21, SPLIT_BINS, 3, 16, False), (3, 1, 1, 9, True)):
        for variant in (0, 1, 2):
            rc, text = describe(L, 3000 * C_, 7, n_pairs, C_, with_std, bits, bins, variant)
            if plan_of(n_pairs, bins, C_, bits, with_std, variant) is None:
                assert rc == nat.HM_EUNSUPPORTED and text == ""
            elif lib == "host":
                assert rc == nat.HM_OK and text == f"host_pairs_hist_dn<dn={'u8' if bits == 8 else 'u16'},bits={bits},std={int(with_std)}>"
            else:
                assert rc == nat.HM_OK and text == describe_of(n_pairs, bins, C_, bits, with_std, variant), (text, n_pairs, bins, C_, bits, variant)
    E = nat.HM_EINVAL
    ok = dict(n=30, nf=3, npairs=3, C_=3, with_std=1, bits=8, bins=8, variant=0)
    for change in (dict(n=0), dict(n=31), dict(C_=0), dict(C_=5), dict(nf=0), dict(nf=nat.HM_MAX_FRAMES + 1), dict(npairs=0), dict(bits=7),
                   dict(bits=17), dict(variant=-1), dict(variant=3), dict(bins=0), dict(bins=nat.HM_PAIRS_HIST_MAX_BINS + 1)):
        assert describe(L, **dict(ok, **change))[0] == E, change
    assert L.hm_pairs_histogram_dn_describe(30, 3, 3, 3, 1, 8, 8, 0, None, 0) == E
    small = C.create_string_buffer(8)
    assert L.hm_pairs_histogram_dn_describe(30, 3, 3, 3, 1, 8, 8, 0, small, len(small)) == nat.HM_OK and len(small.value) < 8


def test_symbols():
    with nat.host_mode():
        host = nat.host_lib()
    for name in SYMBOLS:
        assert hasattr(nat.hip_lib, name) and hasattr(host, name), name
    assert nat.hip_lib.hm_pairs_histogram_dn_workspace_bytes(15, 256, 3, 12) >= nat.hip_lib.hm_pairs_histogram_workspace_bytes(15, 256, 3) + 16 * 4096 * 3
    assert nat.hip_lib.hm_pairs_histogram_dn_workspace_bytes(-1, 0, 9, 99) > 0


# ------------------------------------------------------------------------------------------------ raw calls
class DnArgs:
    """The host-side argument arrays of one call on DN frames; tensors are kept alive here."""

    def __init__(self, device, frames_t, tabs, pairs, with_std):
        self.f = frames_t
        self.bits = int(np.log2(tabs[0].shape[0]))
        self.t = [dn.T(tabs[0], device), dn.T(tabs[1], device) if with_std else None, dn.T(tabs[2], device) if with_std else None]
        self.P = len(pairs)
        self.fp = C.cast((C.c_void_p * len(self.f))(*[t.data_ptr() for t in self.f]), C.POINTER(C.c_void_p))
        self.pi = (C.c_int32 * self.P)(*[p[0] for p in pairs])
        self.pj = (C.c_int32 * self.P)(*[p[1] for p in pairs])
        self.pm = (C.c_double * self.P)(*[p[2] for p in pairs])

    def tp(self, k):
        return None if self.t[k] is None else self.t[k].data_ptr()


def raw_minmax_dn(device, a, C_, thr=None, variant=0, expect=nat.HM_OK):
    with backend(device) as (lib, stream):
        lo, hi = ph.limits(thr, C_)
        out = torch.full((a.P * 2 * C_ * 2,), float("nan"), dtype=torch.float64, device=device)
        ws = torch.empty(max(8, lib.hm_pairs_histogram_dn_workspace_bytes(a.P, 1, C_, a.bits) // 8 + 1), dtype=torch.float64, device=device)
        rc = lib.hm_pairs_minmax_dn(a.fp, len(a.f), a.bits, a.tp(0), a.tp(1), a.tp(2), a.pi, a.pj, a.pm, a.P, a.f[0].numel(), C_, lo, hi, variant,
                                    out.data_ptr(), ws.data_ptr(), stream)
        assert rc == expect, (rc, expect)
        return out.cpu().numpy().reshape(a.P, 2, C_, 2)


def raw_hist_dn(device, a, C_, mask, bins, edges, thr=None, variant=0, prefill=float("nan"), expect=nat.HM_OK):
    """hm_pairs_histogram_dn called directly -> out (P, 2, C, bins) over a `prefill`ed buffer (left untouched when `expect` is an error)."""
    with backend(device) as (lib, stream):
        lo, hi = ph.limits(thr, C_)
        e = dn.T(edges, device)
        out = torch.full((a.P * 2 * C_ * bins,), prefill, dtype=torch.float64, device=device)
        ws = torch.empty(max(8, lib.hm_pairs_histogram_dn_workspace_bytes(a.P, bins, C_, a.bits) // 8 + 1), dtype=torch.float64, device=device)
        rc = lib.hm_pairs_histogram_dn(a.fp, len(a.f), a.bits, a.tp(0), a.tp(1), a.tp(2), a.pi, a.pj, a.pm, a.P, a.f[0].numel(), C_, mask, lo, hi,
                                       e.data_ptr(), bins, variant, out.data_ptr(), ws.data_ptr(), stream)
        assert rc == expect, (rc, expect)
        return out.cpu().numpy().reshape(a.P, 2, C_, bins)


# ------------------------------------------------------------------------------------------------ the oracle
def mapped(frames, tabs, bits, C_, with_std):
    """Part 1's operands: (npix, C) float64 value (and std) arrays of every frame through the tables."""
    icrf, diff, std = tabs
    cols = np.arange(C_)[None, :]
    vals, stds = [], []
    with np.errstate(all="ignore"):
        sd = diff * std if with_std else None                                     # one rounding, as hm_linearize_* multiplies
    for f in frames:
        idx = f.reshape(-1, C_).astype(np.int64) & (2 ** bits - 1)
        vals.append(icrf[idx, cols])
        if with_std:
            stds.append(sd[idx, cols])
    return vals, stds if with_std else None


def linearized(device, frames, tabs, bits, with_std):
    """Part 2's operands: float64 frames (and std frames) of the same backend's linearize, flat tensors."""
    icrf, diff, std = tabs
    bd = None if bits == 8 else bits
    vals, stds = [], []
    with backend(device):
        for f in frames:
            ft = dn.T(f, device)
            if with_std:
                v, s = engine.linearize(ft, engine.linearize(ft, None, std, bit_depth=bd)[0], icrf, diff, bit_depth=bd)
                stds.append(s.reshape(-1))
            else:
                v = engine.linearize(ft, None, icrf, bit_depth=bd)[0]
            vals.append(v.reshape(-1))
    return vals, stds if with_std else None


class Case:
    """One set of inputs with both parts of its oracle, computed once and shared by every variant and placement checked on it."""

    def __init__(self, device, frames, tabs, pairs, with_std, bins, rng=None, mask=None, thr=None, what="case"):
        self.device, self.frames, self.tabs, self.pairs, self.with_std, self.bins, self.thr, self.what = device, frames, tabs, pairs, with_std, bins, thr, what
        self.bits = int(np.log2(tabs[0].shape[0]))
        self.C = C_ = frames[0].shape[-1]
        self.mask = (1 << C_) - 1 if mask is None else mask
        vals, stds = mapped(frames, tabs, self.bits, C_, with_std)
        self.refs, self.mm = [], np.empty((len(pairs), 2, C_, 2))
        ranges = np.empty((len(pairs), 2, C_, 2))
        for p, (i, j, m) in enumerate(pairs):
            d = diff_reference(vals[i], stds[i] if with_std else None, vals[j], stds[j] if with_std else None, m,
                               None if thr is None else thr[0], None if thr is None else thr[1])
            self.refs.append(d)
            for k in range(2):
                for c in range(C_):
                    x, s = d[2 * k][:, c], d[2 * k + 1][:, c] if with_std else None
                    xs = x[counted(x, s)]
                    self.mm[p, k, c] = (xs.min(), xs.max()) if xs.size else (np.inf, -np.inf)
                    ranges[p, k, c] = default_range(x, s) if rng is None else rng
        self.ranges, self.edges = ranges, linspace_edges(ranges, bins)
        self.hist = {(p, k, c): hist_reference(self.refs[p][2 * k][:, c], self.refs[p][2 * k + 1][:, c] if with_std else None, bins, tuple(ranges[p, k, c]))
                     for p in range(len(pairs)) for k in range(2) for c in range(C_) if (self.mask >> c) & 1}
        # part 2, on (fresh) float64 frames of the same backend
        lv, ls = linearized(device, frames, tabs, self.bits, with_std)
        with backend(device):
            fa = ph.Args(device, None, None, pairs, tensors=lv, std_tensors=ls)
        self.f64_mm = ph.raw_minmax(device, None, None, pairs, C_, thr, args=fa)
        self.f64_hist = ph.raw_hist(device, None, None, pairs, C_, self.mask, bins, self.edges, thr, args=fa)

    def check(self, variant=0, place=dn.T, frames=None):
        """Both entries on the DN frames (placed by `place`) against both parts of the oracle -> (histograms, worst error / bound)."""
        device, C_, weighted, what = self.device, self.C, self.with_std, f"{self.what} variant {variant}"
        frames_t = [place(f, device) for f in (self.frames if frames is None else frames)]
        before = [f.clone() for f in frames_t]
        with backend(device):
            a = DnArgs(device, frames_t, self.tabs, self.pairs, weighted)
        mm = raw_minmax_dn(device, a, C_, self.thr, variant)
        assert np.array_equal(mm, self.mm), f"{what}: min / max against the reference"
        assert np.array_equal(mm.view(np.int64), self.f64_mm.view(np.int64)), f"{what}: min / max against the float64 route"
        got = raw_hist_dn(device, a, C_, self.mask, self.bins, self.edges, self.thr, variant)
        for f, b in zip(frames_t, before):
            assert torch.equal(f, b), f"{what}: a DN frame was modified"
        if not weighted:
            assert torch.equal(torch.from_numpy(got), torch.from_numpy(self.f64_hist)), f"{what}: counts against the float64 route"
        worst = 0.0
        fam = family(device, "pairs histogram dn")
        for p in range(len(self.pairs)):
            for k in range(2):
                for c in range(C_):
                    if not (self.mask >> c) & 1:
                        assert np.all(got[p, k, c] == 0.0), f"{what}: channel {c} outside the mask is not 0.0"
                        continue
                    ref = self.hist[p, k, c]
                    h = got[p, k, c] if weighted else got[p, k, c].astype(np.int64)
                    assert weighted or np.array_equal(h, got[p, k, c])                  # counts are whole numbers
                    label = f"{what}: pair {p} kind {k} channel {c}"
                    worst = max(worst, assert_hist(fam, h, self.edges[p, k, c], ref, weighted, label))
                    if weighted:
                        same_weighted(device, h, self.f64_hist[p, k, c], ref, label)
        return got, worst


def same_weighted(device, h, other, ref, what, fam="pairs dn - float64 route"):
    """Two weighted histograms that are each within the bound of the reference: the same NaN / inf pattern, within twice the bound."""
    np.testing.assert_array_equal(np.isnan(h), np.isnan(other))
    np.testing.assert_array_equal(np.isinf(h), np.isinf(other))
    fin = np.isfinite(ref["wsum"]) & (ref["k"] > 0) & np.isfinite(ref["wabs"]) & (ref["wabs"] > 0)
    if fin.any():
        worst = record(family(device, fam), np.abs(h[fin].astype(LD) - other[fin].astype(LD)), 2 * (ref["k"][fin] + 2) * LD(U) * ref["wabs"][fin])
        assert worst <= 1.0, f"{what}: {worst:.3f} x twice the bound"


def frames_of(bits, C_, npix, n_frames, stray=False):
    return [f.reshape(-1, C_) for f in dn.dn_frames(bits, C_, npix * C_, n_frames, stray)]


def ratio_pairs(n_frames, n_pairs=None):
    """(i < j) pairs with multipliers near the ratio of the frames' mean values (random DNs: about 1), so both differences spread."""
    return [(i, j, 1.0 + 0.01 * ((i + 2 * j) % 7)) for i, j, _ in dn.pair_list(n_frames, n_pairs or n_frames * (n_frames - 1) // 2)]


# ------------------------------------------------------------------------------------------------ checks (device: "cpu" or "cuda:0")
def check_sizes(device, npix, C_, with_std):
    if npix >= FULL_SWEEP and C_ != 3:
        npix = npix * 3 // C_ + (1 if npix == RAGGED else 0)               # the same element counts for the other channel counts
    nf = 2 if npix == 35 else 3
    Case(device, frames_of(8, C_, npix, nf), dn.tables(8, C_), ratio_pairs(nf), with_std, 32, None if npix > 1 else (-1.0, 1.0),
         what=f"{npix} px C={C_}").check()


FRAMES_PAIRS = ((2, 1, 256), (7, 15, 64), (7, 15, 256), (32, 16, 256))      # frames, pairs, bins: one launch of 1 / of 15, 8 + 7, 8 + 8


def check_frames_pairs(device, n_frames, n_pairs, bins, with_std):
    launches = plan_of(n_pairs, bins, 3, 8, with_std, 0)
    assert len(launches) == (2 if bins == 256 and n_pairs > 1 else 1)
    if n_frames == 32:                                                      # frame 31 against 0..7, frame 0 against 24..30, and (5, 5)
        pairs = [(i, 31, 1.01) for i in range(8)] + [(0, j, 0.99) for j in range(24, 31)] + [(5, 5, 1.0)]
        assert len(pairs) == nat.HM_PAIRS_MAX and len(launches) == 2
    else:
        pairs = ratio_pairs(n_frames, n_pairs)
    Case(device, frames_of(8, 3, 333, n_frames), dn.tables(8, 3), pairs, with_std, bins, (-0.6, 0.6), what=f"{n_frames} frames {n_pairs} pairs").check()


def check_depth(device, bits, with_std):
    """7 frames / 15 pairs at the depth with thresholds that exclude part of every channel; every variant the depth admits."""
    C_, npix = 3, 4001
    frames, thr = frames_of(bits, C_, npix, 7), dn.limits(bits, C_)
    dn.assert_some_excluded(frames, bits, C_, thr)
    case = Case(device, frames, dn.tables(bits, C_), ratio_pairs(7, 15), with_std, 64, None, thr=thr, what=f"{bits} bits")
    check_variants(case)


def check_variants(case):
    """Variants 0 / 1 / 2 against the oracle and each other; variant 1 refused exactly where plan_of says; _describe as plan_of derives it."""
    device, C_, n = case.device, case.C, case.frames[0].size
    results = {}
    for variant in (0, 1, 2):
        plan = plan_of(len(case.pairs), case.bins, C_, case.bits, case.with_std, variant)
        with backend(device) as (lib, _):
            rc, text = describe(lib, n, len(case.frames), len(case.pairs), C_, case.with_std, case.bits, case.bins, variant)
        if plan is None:
            assert rc == nat.HM_EUNSUPPORTED
            with backend(device):
                a = DnArgs(device, [dn.T(f, device) for f in case.frames], case.tabs, case.pairs, case.with_std)
            out = raw_hist_dn(device, a, C_, case.mask, case.bins, case.edges, case.thr, 1, prefill=-5.0, expect=nat.HM_EUNSUPPORTED)
            assert np.all(out == -5.0)
            continue
        assert rc == nat.HM_OK
        if is_cuda(device):
            assert text == describe_of(len(case.pairs), case.bins, C_, case.bits, case.with_std, variant)
        results[variant] = case.check(variant)[0]
    for variant in (1, 2):
        if variant not in results:
            continue
        if not case.with_std:
            assert np.array_equal(results[variant], results[0]), f"{case.what}: variant {variant} against variant 0"
        else:
            for (p, k, c), ref in case.hist.items():
                same_weighted(device, results[variant][p, k, c], results[0][p, k, c], ref, f"{case.what}: variant {variant} against 0", "pairs dn variants")
    return results


def check_bins(device, bins, bits, with_std):
    """C = 4: one pair's histograms at 2048 bins are 128 KiB - the 8-bit table fits beside them, the 12-bit one does not."""
    C_ = 4
    if bins == 2048:
        assert plan_of(3, bins, C_, 8, with_std, 0) == [(1, 16, "lds")] * 3 and plan_of(3, bins, C_, 12, with_std, 1) is None
    case = Case(device, frames_of(bits, C_, 2999 if bins < 1000 else 9000, 3), dn.tables(bits, C_), ratio_pairs(3), with_std, bins, (-0.5, 0.5),
                what=f"bins={bins} C={C_} bits={bits}")
    results = check_variants(case)
    assert (1 in results) == (plan_of(3, bins, C_, bits, with_std, 1) is not None)


def check_misaligned(device, bits, with_std):
    """uint8 frames at an odd address, uint16 frames 2 bytes off 4-byte alignment: the aligned answer."""
    case = Case(device, frames_of(bits, 3, 4001, 3), dn.tables(bits, 3), ratio_pairs(3), with_std, 32, None, thr=dn.limits(bits, 3), what=f"misaligned {bits} bits")
    a, _ = case.check()
    for variant in (0, 2):
        b, _ = case.check(variant, place=dn.misaligned)
        if not with_std:
            assert np.array_equal(a, b)


def check_stray_bits(device, with_std):
    """12 bits: bits set above the depth change nothing."""
    clean, stray = frames_of(12, 3, 4001, 3), frames_of(12, 3, 4001, 3, True)
    assert all(np.array_equal(s & 4095, c) for s, c in zip(stray, clean)) and any((s >> 12).any() for s in stray)
    case = Case(device, clean, dn.tables(12, 3), ratio_pairs(3), with_std, 32, None, thr=dn.limits(12, 3), what="stray bits")
    a, _ = case.check()
    b, _ = case.check(frames=stray)
    if not with_std:
        assert np.array_equal(a, b)


def check_zero_std(device, bits):
    """A zero std-table entry: the elements at which both frames of a pair hold that DN are skipped when weighted and counted when not."""
    tabs = dn.tables(bits, 3, True)
    frames = [f.copy() for f in frames_of(bits, 3, 4001, 3)]
    for f in frames:                                                        # both stds 0 at the same elements: the difference stds are 0
        f[100:150] = 2 ** bits // 3
    weighted = Case(device, frames, tabs, ratio_pairs(3), True, 16, (-2.0, 2.0), what=f"zero std {bits} bits")
    plain = Case(device, frames, tabs, ratio_pairs(3), False, 16, (-2.0, 2.0), what=f"zero std {bits} bits, unweighted")
    weighted.check()
    got, _ = plain.check()
    assert all(plain.hist[key]["inrange"] > weighted.hist[key]["inrange"] for key in plain.hist)
    assert got.sum() == sum(r["inrange"] for r in plain.hist.values())


def special_tables(C_):
    """8-bit tables with NaN / +-inf / 0 value rows and inf / NaN std rows (copies: the cached ones stay as they are)."""
    icrf, diff, std = (t.copy() for t in dn.tables(8, C_))
    icrf[5], icrf[9], icrf[11], icrf[13] = np.nan, np.inf, -np.inf, 0.0
    std[17], std[19] = np.inf, np.nan
    return icrf, diff, std


def check_specials(device, with_std):
    frames = frames_of(8, 3, 4001, 3)
    assert all(all((f == row).any() for row in (5, 9, 11, 13, 17, 19)) for f in frames)
    for rng in ((-1.0, 1.0), None):
        Case(device, frames, special_tables(3), ratio_pairs(3), with_std, 8, rng, what="NaN / inf table rows").check()


def check_masks(device, with_std):
    frames, tabs = frames_of(8, 4, 411, 3), dn.tables(8, 4)
    for mask in (0b0001, 0b1010, 0b0110, 0b0000):
        Case(device, frames, tabs, ratio_pairs(3), with_std, 16, (-0.5, 0.5), mask=mask, thr=dn.limits(8, 4), what=f"mask {mask:04b}").check()


def edge_tables(lo, hi, bins, C_, kind):
    """test_pairs_hist_host's edge cases as DN frames: a table whose rows are the case's distinct x values (the same in every channel) and,
    in its last row, the case's constant y; frame 0 holds each element's row, frame 1 the last row. -> bits, frames, tables, stds' rng."""
    x, y, rng = ph.edge_case(lo, hi, bins, C_, kind)
    values, inverse = np.unique(x.ravel(), return_inverse=True)
    bits = next(b for b in (8, 10, 12, 16) if 2 ** b > values.size)
    rows = 2 ** bits
    icrf = np.full((rows, C_), 0.5)
    icrf[:values.size] = values[:, None]
    icrf[rows - 1] = y.ravel()[0]
    dtype = np.uint8 if bits == 8 else np.uint16
    frames = [inverse.astype(dtype).reshape(x.shape), np.full(x.shape, rows - 1, dtype)]
    diff = np.ones((rows, C_))
    std = 0.05 + rng.random((rows, C_))
    assert np.array_equal(icrf[frames[0].astype(np.int64), np.arange(C_)[None, :]], x) and np.all(icrf[rows - 1] == y.ravel()[0])
    return bits, frames, (icrf, diff, std)


def check_edges(device, lo, hi, bins, C_, kind, with_std):
    bits, frames, tabs = edge_tables(lo, hi, bins, C_, kind)
    got, _ = Case(device, frames, tabs, [(0, 1, 1.0)], with_std, bins, (lo, hi), what=f"edge values ({lo}, {hi}, {bins}) kind {kind}, {bits} bits").check()
    if kind == 0:
        assert np.all(got[0, 1] == 0.0)                                     # y = 0: every relative difference is non-finite


def check_flat_edges(device):
    """A (pair, kind, channel) whose last edge is not above its first counts nothing."""
    case = Case(device, frames_of(8, 3, 411, 2), dn.tables(8, 3), [(0, 1, 1.0)], False, 8, (-0.5, 0.5), what="flat edges")
    case.edges[0, 1, 1] = 0.25
    case.edges[0, 0, 2] = case.edges[0, 0, 2][::-1]
    with backend(device):
        a = DnArgs(device, [dn.T(f, device) for f in case.frames], case.tabs, case.pairs, False)
    got = raw_hist_dn(device, a, 3, 7, 8, case.edges)
    assert np.all(got[0, 1, 1] == 0.0) and np.all(got[0, 0, 2] == 0.0) and got[0, 0, 0].sum() == case.hist[0, 0, 0]["inrange"] > 0


def check_status(device, lib=None):
    """Every status in order, `out` pre-filled and untouched on an error: the same codes on both builds (csrc/hm_pairs_rules.h).
    lib: another library to ask with the device's memory - the refusals only, which return before anything is launched."""
    C_, nf, n, bins = 3, 3, 30, 8
    E, A, UNS = nat.HM_EINVAL, nat.HM_EALIGN, nat.HM_EUNSUPPORTED
    refusals_only = lib is not None
    with backend(device) as (own, stream):
        lib = lib or own

        def call(hist=True, bits=8, frames=None, icrf=True, diff=True, std=True, pi=(0, 0, 1), pj=(1, 2, 2), n_=n, C__=C_, nf_=nf, npairs=3, lo=True,
                 hi=True, variant=0, out=True, ws=True, table_off=0, null_frame=False, bins_=bins, mask=7, edges=True, pm=True):
            rows = 2 ** bits
            dt = torch.uint8 if bits == 8 else torch.uint16
            fr = frames if frames is not None else [torch.zeros(n, dtype=dt, device=device) for _ in range(nf)]
            tabs = [torch.ones(rows * 4 + 1, dtype=torch.float64, device=device) for _ in range(3)]
            o = torch.full((3 * 2 * 4 * 2048,), 7.0, dtype=torch.float64, device=device)
            e = torch.linspace(0.0, 2.0, 2049, dtype=torch.float64, device=device).repeat(3 * 2 * 4)
            w = torch.zeros(max(1, lib.hm_pairs_histogram_dn_workspace_bytes(3, bins, 4, bits) // 8 + 1), dtype=torch.float64, device=device)
            fp = (C.c_void_p * len(fr))(*[f.data_ptr() for f in fr])
            if null_frame:
                fp[1] = None
            tp = [t.data_ptr() + table_off if use else None for t, use in zip(tabs, (icrf, diff, std))]
            lim = (C.c_double * 4)(0.1, 0.1, 0.1, 0.1), (C.c_double * 4)(0.9, 0.9, 0.9, 0.9)
            common = (C.cast(fp, C.POINTER(C.c_void_p)), nf_, bits, tp[0], tp[1], tp[2], (C.c_int32 * 3)(*pi), (C.c_int32 * 3)(*pj),
                      (C.c_double * 3)(0.5, 0.25, 0.5) if pm else None, npairs, n_, C__)
            tail = (o.data_ptr() if out else None, w.data_ptr() if ws else None, stream)
            if hist:
                rc = lib.hm_pairs_histogram_dn(*common, mask, lim[0] if lo else None, lim[1] if hi else None, e.data_ptr() if edges else None, bins_,
                                               variant, *tail)
            else:
                rc = lib.hm_pairs_minmax_dn(*common, lim[0] if lo else None, lim[1] if hi else None, variant, *tail)
            if is_cuda(device):
                torch.cuda.synchronize()
            assert bool((o == 7.0).all()) == (rc != nat.HM_OK), ("out touched on an error, or untouched on success", rc)
            return rc
        for hist in (True, False):
            if not refusals_only:
                assert call(hist) == nat.HM_OK and call(hist, bits=12) == nat.HM_OK and call(hist, std=False, diff=False) == nat.HM_OK
                assert call(hist, bits=10, variant=1) == nat.HM_OK and call(hist, bits=12, variant=2) == nat.HM_OK and call(hist, std=False) == nat.HM_OK
                odd8 = [torch.zeros(n + 1, dtype=torch.uint8, device=device)[1:] for _ in range(nf)]
                assert call(hist, frames=odd8) == nat.HM_OK                        # uint8 frames have no alignment rule
            for kw in (dict(n_=0), dict(n_=31), dict(C__=0), dict(C__=5, n_=30, mask=1), dict(nf_=0), dict(nf_=nat.HM_MAX_FRAMES + 1), dict(npairs=0),
                       dict(lo=False), dict(hi=False), dict(icrf=False), dict(out=False), dict(ws=False), dict(pm=False), dict(bits=7), dict(bits=17),
                       dict(variant=3), dict(variant=-1), dict(diff=False), dict(null_frame=True), dict(pi=(0, 3, 1)), dict(pj=(1, -1, 2))):
                assert call(hist, **kw) == E, kw
            assert call(hist, table_off=4) == A
            odd16 = [torch.zeros(n + 1, dtype=torch.uint16, device=device).view(torch.uint8)[1:2 * n + 1] for _ in range(nf)]
            assert all(f.data_ptr() % 2 == 1 for f in odd16)
            assert call(hist, bits=12, frames=odd16) == A
            assert call(hist, bits=12, frames=odd16, pi=(0, 3, 1)) == A             # the alignment rule comes before the pair indices
            assert call(hist, table_off=4, bits=17) == E                            # ... and after the depth
            assert call(hist, bits=16, variant=1) == UNS                            # 1.5 MiB of table
            assert call(hist, bits=16, variant=1, pj=(1, 9, 2)) == E                # a pair index before the table that does not fit
        # the histogram's own rules: after the pair indices, before the fit rule
        for kw in (dict(bins_=0), dict(bins_=nat.HM_PAIRS_HIST_MAX_BINS + 1), dict(mask=8), dict(mask=-1), dict(edges=False)):
            assert call(True, **kw) == E, kw
            assert call(True, bits=16, variant=1, **kw) == E, kw
            assert call(True, table_off=4, **kw) == A and call(True, pi=(0, 3, 1), **kw) == E, kw
        assert call(True, bits=12, variant=1, C__=4, n_=32, mask=15, bins_=2048) == UNS
        if not refusals_only:
            assert call(True, mask=0) == nat.HM_OK and call(True, lo=False, hi=False) == nat.HM_OK and call(False, bits=12, variant=1, std=False, diff=False) == nat.HM_OK


# ------------------------------------------------------------------------------------------------ the Python layer
def check_engine(device, bits, with_std):
    """engine.pairs_histogram_dn against engine.pairs_histogram on linearized frames: the same edges (included_range None: through the min /
    max pass), dtypes and channels; counts equal, weighted bins within twice the bound (a relative 2 (npix + 3) u: the weights are > 0)."""
    C_, npix, nf = 3, 2001, 4
    tabs, thr = dn.tables(bits, C_), dn.limits(bits, C_)
    frames = frames_of(bits, C_, npix, nf)
    pairs = ratio_pairs(nf)
    icrf, diff, std = tabs
    lv, ls = linearized(device, frames, tabs, bits, with_std)
    kw = dict(bit_depth=None if bits == 8 else bits)
    with backend(device):
        frames_t = [dn.T(f.reshape(npix, 1, C_), device) for f in frames]
        before = [f.clone() for f in frames_t]
        for rng, channels, variant in ((None, None, 0), ((-0.3, 0.3), [2, 0], 2), (None, [1], 0)):
            got = engine.pairs_histogram_dn(frames_t, pairs, icrf, diff if with_std else None, std if with_std else None, bins=48, included_range=rng,
                                            channels=channels, thresholds=thr, variant=variant, **kw)
            want = engine.pairs_histogram([v.view(npix, 1, C_) for v in lv], None if ls is None else [s.view(npix, 1, C_) for s in ls], pairs, 48, rng,
                                          [0, 1, 2] if channels is None else channels, thresholds=thr)
            ph.same_distributions(got, want, with_std, npix)
        for f, b in zip(frames_t, before):
            assert torch.equal(f, b)


def check_value_errors(device):
    C_, n = 3, 30
    icrf, diff, std = dn.tables(8, C_)
    f8 = [torch.zeros((n // C_, 1, C_), dtype=torch.uint8, device=device) for _ in range(2)]
    f16 = [torch.zeros((n // C_, 1, C_), dtype=torch.uint16, device=device) for _ in range(2)]
    pairs = [(0, 1, 0.5)]
    with backend(device):
        for frames, kw in ((f8, dict(bit_depth=8)), (f16, dict()), (f16, dict(bit_depth=8)), (f16, dict(bit_depth=17)), ([f8[0], f16[0]], dict()),
                           ([f8[0], f8[1][:5]], dict()), (f8, dict(icrf=dn.tables(10, C_)[0])), (f16, dict(bit_depth=10)),
                           (f8, dict(std_table=std, icrf_diff=None)), (f8, dict(std_table=std[:100])), (f8, dict(icrf_diff=diff[:, :2])),
                           (f8, dict(thresholds=([0.1], [0.9]))), ([f.to(torch.float64) for f in f8], dict()), (f8, dict(bins=0)),
                           (f8, dict(bins=nat.HM_PAIRS_HIST_MAX_BINS + 1)), (f8, dict(channels=[3])), (f8, dict(included_range=(1.0, 0.0))),
                           (f8, dict(variant=-1)), (f8, dict(variant=3)), ([], dict())):
            args = dict(icrf=icrf, icrf_diff=diff, std_table=None, bins=8)
            args.update(kw)
            with pytest.raises(ValueError):
                engine.pairs_histogram_dn(frames, pairs, args.pop("icrf"), **args)
        with pytest.raises(NotImplementedError):
            t12 = dn.tables(12, 4)
            f = [torch.zeros((8, 1, 4), dtype=torch.uint16, device=device) for _ in range(2)]
            engine.pairs_histogram_dn(f, pairs, t12[0], bins=2048, included_range=(0.0, 1.0), bit_depth=12, variant=1)
        with pytest.raises(ValueError):                                        # engine.pairs_histogram keeps refusing DN frames
            engine.pairs_histogram(f8, None, pairs, 8, (0.0, 1.0), [0])


def check_series(device, use_std):
    """ExposureSeries.process_linearity_distribution(from_dn=True) against linearize-then-distribution on a deep copy; the series stays DN
    frames and the copy's route is the float64 one."""
    assert gs.NUM_OF_CHS == 3
    icrf, diff, std = dn.tables(8, 3)
    shape = (24, 17, 3)
    series = dn.make_series(device, 4, shape)
    lower, upper = [0.05, None, 0.1], [0.7, 0.5, None]
    for rng, channels, lo, hi in (((-0.3, 0.3), None, None, None), (None, [2, 0], None, None), (None, None, lower, upper)):
        ref = copy.deepcopy(series)
        dns = [s.measurand._dn.clone() for s in series.input_image_sets]
        got = series.process_linearity_distribution(48, rng, channels, use_std, lower=lo, upper=hi, from_dn=True, ICRF=icrf, ICRF_diff=diff, STD_data=std)
        for s, d in zip(series.input_image_sets, dns):
            m = s.measurand
            assert m._dn is not None and torch.equal(m._dn, d) and m._val is None and m._std is None
        if use_std:
            for s in ref.input_image_sets:
                s.measurand.std = s.calculate_numerical_STD(std)
        lin = ref.linearize(icrf, diff)
        lin.initialize_exposure_pairs()
        want = lin.process_linearity_distribution(48, rng, channels, use_std, lower=lo, upper=hi)
        assert len(got) == len(series.exposure_pairs) == 6
        ph.same_distributions(got, want, use_std, shape[0] * shape[1])
        assert any(h.sum() > 0 for ab, rel in got for d in (ab, rel) for h, _ in d.values())


def check_series_errors(device):
    icrf, diff, std = dn.tables(8, 3)
    series = dn.make_series(device, 3, (8, 5, 3))
    with pytest.raises(ValueError, match="needs ICRF"):
        series.process_linearity_distribution(8, None, None, False, from_dn=True)
    with pytest.raises(ValueError, match="ICRF_diff and STD_data"):
        series.process_linearity_distribution(8, None, None, True, from_dn=True, ICRF=icrf, ICRF_diff=diff)
    with pytest.raises(ValueError, match="ICRF_diff and STD_data"):
        series.process_linearity_distribution(8, None, None, True, from_dn=True, ICRF=icrf, STD_data=std)
    with pytest.raises(ValueError, match="must match the size"):
        series.process_linearity_distribution(8, None, None, False, lower=[0.1], upper=[0.9], from_dn=True, ICRF=icrf)
    with_std = copy.deepcopy(series)
    for s in with_std.input_image_sets:
        s.measurand.std = np.full((8, 5, 3), 0.01)
    with pytest.raises(ValueError, match="default route"):
        with_std.process_linearity_distribution(8, None, None, True, from_dn=True, ICRF=icrf, ICRF_diff=diff, STD_data=std)
    lin = series.linearize(icrf)
    lin.initialize_exposure_pairs()
    with pytest.raises(ValueError, match="from_dn measurand"):
        lin.process_linearity_distribution(8, None, None, False, from_dn=True, ICRF=icrf)
    no_pairs = dn.make_series(device, 3, (8, 5, 3))
    no_pairs.exposure_pairs = None
    with pytest.raises(ValueError, match="own images"):
        no_pairs.process_linearity_distribution(8, None, None, False, from_dn=True, ICRF=icrf)


# ------------------------------------------------------------------------------------------------ the host build
DEV = "cpu"
STD = pytest.mark.parametrize("with_std", [False, True])


@STD
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
@pytest.mark.parametrize("name,npix", SIZES)
def test_sizes(name, npix, C_, with_std):
    check_sizes(DEV, npix, C_, with_std)


@STD
@pytest.mark.parametrize("n_frames,n_pairs,bins", FRAMES_PAIRS)
def test_frames_pairs(n_frames, n_pairs, bins, with_std):
    check_frames_pairs(DEV, n_frames, n_pairs, bins, with_std)


@STD
@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_depths(bits, with_std):
    check_depth(DEV, bits, with_std)


@STD
@pytest.mark.parametrize("bits", [8, 12])
@pytest.mark.parametrize("bins", BINS)
def test_bins(bins, bits, with_std):
    check_bins(DEV, bins, bits, with_std)


@STD
@pytest.mark.parametrize("bits", [8, 12])
def test_misaligned(bits, with_std):
    check_misaligned(DEV, bits, with_std)


@STD
def test_stray_bits(with_std):
    check_stray_bits(DEV, with_std)


@pytest.mark.parametrize("bits", [8, 12])
def test_zero_std(bits):
    check_zero_std(DEV, bits)


@STD
def test_specials(with_std):
    check_specials(DEV, with_std)


@STD
def test_masks(with_std):
    check_masks(DEV, with_std)


@STD
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("lo,hi,bins,C_", EDGE_SETS)
def test_edges(lo, hi, bins, C_, kind, with_std):
    check_edges(DEV, lo, hi, bins, C_, kind, with_std)


def test_flat_edges():
    check_flat_edges(DEV)


def test_status_host_build():
    check_status(DEV)


def test_status_device_build_without_gpu():
    """The device build's refusals return before anything is launched, written or dereferenced: they can be asked for with host memory."""
    check_status(DEV, lib=nat.hip_lib)


@STD
@pytest.mark.parametrize("bits", [8, 12])
def test_engine(bits, with_std):
    check_engine(DEV, bits, with_std)


def test_value_errors():
    check_value_errors(DEV)


@STD
def test_series(with_std):
    check_series(DEV, with_std)


def test_series_errors():
    check_series_errors(DEV)
