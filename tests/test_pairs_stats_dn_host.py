"""hm_pairs_statistics_dn / engine.pairs_statistics_dn / ExposureSeries.process_linearity(from_dn=True): the all-pairs linearity statistics
straight from uint8 and uint16 DN frames, on the HOST build (csrc_host/hm_host.cpp). The checks are functions of a device name:
tests/test_gpu_pairs_stats_dn.py runs the same ones on the MI355X.

The oracle is the route the entry replaces, on the same build and device: every frame materialised with engine.linearize(f, None, icrf) -
with stds engine.linearize(f, engine.linearize(f, None, std_table)[0], icrf, icrf_diff) - then engine.pairs_statistics(vals, stds, pairs,
thresholds=...) on those (fresh) float64 frames. The new entry evaluates the same element values - ICRF[DN, c], ICRF_diff[DN, c] *
STD_table[DN, c], NaN where apply_thresholds excludes the value - and feeds them to the same pair arithmetic in the same order, so the
results are compared BIT FOR BIT (torch.equal on the int64 view of the raw outputs: NaNs compare as bits). The DN frames must be
byte-identical after every call.

Inputs: per-channel ICRF columns that differ (x ** (1 + 0.35 c)), a non-monotone positive std_table (one case with a zero entry), random DNs
over the full range of the depth. Every thresholded case asserts from its own inputs that, per channel, some but not all elements are
excluded. Shapes: the smallest that reach every path - the grid is stat_grid(n, 64), at most 768 workgroups of one 64-element chunk, two
chunks per iteration: n = C (one partial chunk), 768 (no whole iteration), 196 608 (exactly two whole iterations of the full grid), 197 052
(whole iterations, partial chunks and a tail)."""
import contextlib
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from camera_linearity_amd import settings as gs
from camera_linearity_amd.exposure_series import ExposureSeries
from camera_linearity_amd.image_set import ImageSet

SIZES = (1, 12 * 64, 196608, 197052)                  # x C for n = C; the others are divisible by 1..4 as they stand
N_BIG = 197052
SHAPES = ((2, 1), (3, 3), (7, 15), (7, 4), (7, 21), (32, 16))        # frames, pairs
SYMBOLS = ("hm_pairs_statistics_dn_workspace_bytes", "hm_pairs_statistics_dn", "hm_pairs_statistics_dn_describe")


# ------------------------------------------------------------------------------------------------ plumbing
def is_cuda(device):
    return str(device).startswith("cuda")


@contextlib.contextmanager
def backend(device):
    """-> (the library that computes on `device`, the stream argument of its entry points)."""
    if is_cuda(device):
        with torch.cuda.device(device):
            yield nat.hip_lib, nat.current_stream_ptr(torch.device(device))
    else:
        with nat.host_mode():
            yield nat.host_lib(), None


def n_of(size, C_):
    return C_ if size == 1 else size


@functools.lru_cache(maxsize=None)
def tables(bits, C_, zero_std=False):
    """(icrf, icrf_diff, std_table), each (2**bits, C) float64: monotone ICRF columns that differ per channel, their derivative, a
    non-monotone positive std table (zero_std: one entry of every channel is 0)."""
    rows = 2 ** bits
    x = np.arange(rows, dtype=np.float64) / (rows - 1)
    icrf = np.stack([x ** (1.0 + 0.35 * c) for c in range(C_)], axis=1)
    diff = np.stack([np.gradient(icrf[:, c], 2.0 / (rows - 1)) for c in range(C_)], axis=1) + 0.05
    k = np.arange(rows, dtype=np.float64)[:, None] * (256.0 / rows)
    std = 0.004 + 0.003 * np.sin(0.37 * k + np.arange(C_)[None, :]) ** 2 + 0.001 * ((k.astype(np.int64) * 7) % 5)
    if zero_std:
        std[rows // 3] = 0.0
    return icrf, diff, std                                                 # (cached: nothing writes them)


def limits(bits, C_):
    """apply_thresholds limits in ICRF units: rows at 8 % and 90 % of the depth, per channel (they differ with the columns)."""
    icrf = tables(bits, C_)[0]
    rows = 2 ** bits
    return [float(icrf[int(0.08 * rows), c]) for c in range(C_)], [float(icrf[int(0.90 * rows), c]) for c in range(C_)]


@functools.lru_cache(maxsize=None)
def dn_frames(bits, C_, n, n_frames, stray=False):
    """n_frames host arrays of n random DNs over the full range of the depth, shaped (n / C, 1, C). The first pixel of frame 0 is DN 0
    (excluded by any lower limit) and of the last frame the middle DN (never excluded), so that the smallest case has both kinds.
    stray: uint16 frames with random bits set above the depth."""
    rng = np.random.default_rng(1000 * bits + 100 * C_ + n_frames + n)
    rng_stray = np.random.default_rng(5)
    rows = 2 ** bits
    out = []
    for i in range(n_frames):
        f = rng.integers(0, rows, size=(n // C_, 1, C_)).astype(np.uint8 if bits == 8 else np.uint16)
        if i == 0:
            f[0] = 0
        if i == n_frames - 1:
            f[0] = rows // 2
        if stray:
            f |= (rng_stray.integers(0, 2 ** (16 - bits), size=f.shape).astype(np.uint16) << bits)
        f.setflags(write=False)
        out.append(f)
    return tuple(out)


def pair_list(n_frames, n_pairs):
    """The first n_pairs of all (i < j) pairs - and, past those (32 frames / 16 pairs takes none, 2 / 1 has one), none twice."""
    allp = [(i, j, 0.5 ** (0.25 * (j - i))) for i in range(n_frames) for j in range(i + 1, n_frames)]
    assert len(allp) >= n_pairs
    return allp[:n_pairs]


def T(a, device):
    return torch.tensor(np.ascontiguousarray(a), device=device)            # (a copy: the cases' arrays are never modified)


def misaligned(a, device):
    """The DNs of `a` at an odd address (uint8) or at a 2-byte but not 4-byte aligned one (uint16): not item-aligned."""
    a = np.ascontiguousarray(a)
    big = torch.zeros(a.size + 4, dtype=torch.uint8 if a.dtype == np.uint8 else torch.uint16, device=device)
    item = a.dtype.itemsize
    k = next(k for k in range(4) if (big.data_ptr() + k * item) % (2 * item) == item)
    view = big[k:k + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    assert view.data_ptr() % (2 * item) == item and view.is_contiguous()
    return view


def assert_some_excluded(frames, bits, C_, thr):
    icrf = tables(bits, C_)[0]
    mask = 2 ** bits - 1
    for c in range(C_):
        v = np.concatenate([icrf[(f[..., c].astype(np.int64) & mask).ravel(), c] for f in frames])
        ex = (v < thr[0][c]) | (v > thr[1][c])
        assert 0 < ex.sum() < ex.size, (c, int(ex.sum()), ex.size)


def raw(stats):
    """The raw outputs of a pairs_statistics result as one int64 tensor (error: present or None alike on both routes)."""
    parts = []
    for ab, rel in stats:
        for d in (ab, rel):
            for k in ("mean", "std", "error"):
                if d[k] is not None:
                    parts.append(d[k].reshape(-1))
    return torch.cat(parts).contiguous().view(torch.int64)


def same_bits(got, ref, what=""):
    for (ga, gr), (ra, rr) in zip(got, ref):
        assert (ga["error"] is None) == (ra["error"] is None) and (gr["error"] is None) == (rr["error"] is None)
    g, r = raw(got).cpu(), raw(ref).cpu()
    assert g.shape == r.shape and torch.equal(g, r), (what, int((g != r).sum()), g.numel())


def oracle(device, frames_t, bits, C_, pairs, with_std, thr, zero_std=False):
    """The parent's route on the same build and device: N x linearize, then pairs_statistics with in-place thresholds on those frames."""
    icrf, diff, std = tables(bits, C_, zero_std)
    bd = None if bits == 8 else bits
    with backend(device):
        vals, stds = [], []
        for f in frames_t:
            if with_std:
                s0 = engine.linearize(f, None, std, bit_depth=bd)[0]
                v, s = engine.linearize(f, s0, icrf, diff, bit_depth=bd)
                stds.append(s)
            else:
                v = engine.linearize(f, None, icrf, bit_depth=bd)[0]
            vals.append(v)
        return engine.pairs_statistics(vals, stds if with_std else None, pairs, thresholds=thr)


def run_dn(device, frames_t, bits, C_, pairs, with_std, thr, variant=0, zero_std=False):
    """engine.pairs_statistics_dn on the frames; they must come back byte-identical."""
    icrf, diff, std = tables(bits, C_, zero_std)
    before = [f.clone() for f in frames_t]
    with backend(device):
        got = engine.pairs_statistics_dn(frames_t, pairs, icrf, diff if with_std else None, std if with_std else None, thresholds=thr,
                                         bit_depth=None if bits == 8 else bits, variant=variant)
        if is_cuda(device):
            torch.cuda.synchronize()
    for f, b in zip(frames_t, before):
        assert torch.equal(f, b), "hm_pairs_statistics_dn changed a DN frame"
    return got


def check_case(device, bits, C_, n, n_frames, n_pairs, with_std, with_thr, variant=0, zero_std=False, place=T):
    frames = dn_frames(bits, C_, n, n_frames)
    pairs = pair_list(n_frames, n_pairs)
    thr = limits(bits, C_) if with_thr else None
    if with_thr:
        assert_some_excluded(frames, bits, C_, thr)
    frames_t = [place(f, device) for f in frames]
    got = run_dn(device, frames_t, bits, C_, pairs, with_std, thr, variant, zero_std)
    ref = oracle(device, [T(f, device) for f in frames], bits, C_, pairs, with_std, thr, zero_std)
    same_bits(got, ref, (bits, C_, n, n_frames, n_pairs, with_std, with_thr, variant))
    return got


# ------------------------------------------------------------------------------------------------ checks (device: "cpu" or "cuda:0")
def check_parent_forms(device, with_std):
    """The parent's entry alone: its staged form (16-byte aligned frames) and its per-wave form (frames 8 bytes off) give each other's
    bits on these inputs - so the new entry's two forms may both be held to the one oracle."""
    from test_stats_limits_host import offset_by_8
    bits, C_, n, nf = 8, 3, N_BIG, 7
    pairs = pair_list(nf, 15)
    icrf, diff, std = tables(bits, C_)
    thr = limits(bits, C_)
    res = []
    with backend(device):
        for place in (lambda a: T(a, device), lambda a: offset_by_8(a, device)):
            vals, stds = [], []
            for f in dn_frames(bits, C_, n, nf):
                ft = T(f, device)
                if with_std:
                    v, s = engine.linearize(ft, engine.linearize(ft, None, std)[0], icrf, diff)
                    stds.append(place(s.cpu().numpy()))
                else:
                    v = engine.linearize(ft, None, icrf)[0]
                vals.append(place(v.cpu().numpy()))
            res.append(engine.pairs_statistics(vals, stds if with_std else None, pairs, thresholds=thr))
    same_bits(res[1], res[0], "hm_pairs_statistics: per-wave form against staged form")


def check_shapes(device, size, C_, with_std, with_thr):
    check_case(device, 8, C_, n_of(size, C_), 3, 3, with_std, with_thr)


def check_frames_pairs(device, n_frames, n_pairs, with_std):
    check_case(device, 8, 3, N_BIG, n_frames, n_pairs, with_std, True)


def check_alignment(device, bits, with_std):
    """Frames that are not item-aligned take the per-wave form and give the aligned answer (both equal the oracle's bits)."""
    a = check_case(device, bits, 3, N_BIG, 7, 15, with_std, True)
    b = check_case(device, bits, 3, N_BIG, 7, 15, with_std, True, place=misaligned)
    same_bits(b, a, "misaligned frames")


def check_depth(device, bits, C_, with_std):
    check_case(device, bits, C_, N_BIG, 7, 15, with_std, True)


def check_zero_std(device, bits):
    check_case(device, bits, 3, N_BIG, 3, 3, True, True, zero_std=True)


def check_stray_bits(device, with_std):
    """12 bits: bits set above the depth change nothing."""
    bits, C_, n, nf = 12, 3, N_BIG, 3
    pairs, thr = pair_list(nf, 3), limits(bits, C_)
    clean, stray = dn_frames(bits, C_, n, nf), dn_frames(bits, C_, n, nf, True)
    assert all(np.array_equal(s & 4095, c) for s, c in zip(stray, clean)) and any((s >> 12).any() for s in stray)
    a = run_dn(device, [T(f, device) for f in clean], bits, C_, pairs, with_std, thr)
    b = run_dn(device, [T(f, device) for f in stray], bits, C_, pairs, with_std, thr)
    same_bits(b, a, "stray bits")
    same_bits(b, oracle(device, [T(f, device) for f in stray], bits, C_, pairs, with_std, thr), "stray bits against the oracle")


def check_variants(device, bits, with_std):
    """variant 1 (table in LDS), 2 (global gathers) and -1 (per-wave) agree with the library's choice; a forced variant 1 whose table
    does not fit is refused."""
    fits = (16 if with_std else 8) * 2 ** bits * 3 + 63 * 1024 <= 160 * 1024
    base = check_case(device, bits, 3, N_BIG, 7, 15, with_std, True)
    for variant in (1, 2, -1):
        if variant == 1 and not fits:
            with pytest.raises(NotImplementedError):
                check_case(device, bits, 3, N_BIG, 7, 15, with_std, True, variant=1)
            continue
        same_bits(check_case(device, bits, 3, N_BIG, 7, 15, with_std, True, variant=variant), base, ("variant", variant))


DESCRIBE = (                                          # n_frames, n_pairs, C, with_std, bits, variant, aligned -> the device build's string
    ((7, 15, 3, 1, 8, 0, 1), "pairs_stats_dn_lds<dn=u8,bits=8,tab=lds,std=1,ni=1>"),
    ((7, 15, 3, 0, 8, 0, 1), "pairs_stats_dn_lds<dn=u8,bits=8,tab=lds,std=0,ni=1>"),
    ((7, 15, 3, 1, 10, 0, 1), "pairs_stats_dn_lds<dn=u16,bits=10,tab=lds,std=1,ni=1>"),
    ((7, 15, 3, 1, 12, 0, 1), "pairs_stats_dn_lds<dn=u16,bits=12,tab=global,std=1,ni=1>"),
    ((7, 15, 3, 0, 12, 0, 1), "pairs_stats_dn_lds<dn=u16,bits=12,tab=lds,std=0,ni=1>"),
    ((7, 15, 4, 0, 12, 0, 1), "pairs_stats_dn_lds<dn=u16,bits=12,tab=global,std=0,ni=1>"),
    ((7, 15, 3, 1, 16, 0, 1), "pairs_stats_dn_lds<dn=u16,bits=16,tab=global,std=1,ni=1>"),
    ((2, 1, 3, 1, 8, 0, 1), "pairs_stats_dn_lds<dn=u8,bits=8,tab=lds,std=1,ni=2>"),
    ((3, 3, 3, 1, 8, 0, 1), "pairs_stats_dn_lds<dn=u8,bits=8,tab=lds,std=1,ni=1>"),
    ((7, 4, 3, 1, 8, 0, 1), "pairs_stats_dn_lds<dn=u8,bits=8,tab=lds,std=1,ni=2>"),
    ((7, 21, 3, 1, 8, 0, 1), "pairs_stats_dn_lds<dn=u8,bits=8,tab=lds,std=1,ni=1> + pairs_stats_dn_lds<dn=u8,bits=8,tab=lds,std=1,ni=2>"),
    ((32, 16, 3, 0, 8, 0, 1), "pairs_stats_dn_wave<dn=u8,bits=8,std=0>"),
    ((32, 16, 3, 1, 8, 0, 1), "pairs_stats_dn_wave<dn=u8,bits=8,std=1>"),
    ((7, 15, 3, 1, 8, 0, 0), "pairs_stats_dn_wave<dn=u8,bits=8,std=1>"),
    ((7, 15, 3, 1, 12, 0, 0), "pairs_stats_dn_wave<dn=u16,bits=12,std=1>"),
    ((7, 15, 3, 1, 10, 1, 1), "pairs_stats_dn_lds<dn=u16,bits=10,tab=lds,std=1,ni=1>"),
    ((7, 15, 3, 1, 10, 2, 1), "pairs_stats_dn_lds<dn=u16,bits=10,tab=global,std=1,ni=1>"),
    ((7, 15, 3, 1, 10, -1, 1), "pairs_stats_dn_wave<dn=u16,bits=10,std=1>"),
)


def describe(lib, n, nf, npairs, C_, with_std, bits, variant, aligned):
    buf = C.create_string_buffer(512)
    rc = lib.hm_pairs_statistics_dn_describe(n, nf, npairs, C_, with_std, bits, variant, aligned, buf, len(buf))
    return rc, buf.value.decode()


def check_status(device, lib=None):
    """The argument rules, each with `out` pre-filled and untouched: the same codes on both builds (csrc/hm_pairs_rules.h).
    lib: another library to ask with the device's memory - the refusals only, which return before anything is launched."""
    C_, nf, n = 3, 3, 30
    E, A, U = nat.HM_EINVAL, nat.HM_EALIGN, nat.HM_EUNSUPPORTED
    refusals_only = lib is not None
    with backend(device) as (own, stream):
        lib = lib or own
        def call(bits=8, frames=None, icrf=True, diff=True, std=True, pi=(0, 0, 1), pj=(1, 2, 2), n_=n, C__=C_, nf_=nf, npairs=3, lo=True,
                 hi=True, variant=0, out=True, ws=True, table_off=0, null_frame=False):
            rows = 2 ** bits
            dt = torch.uint8 if bits == 8 else torch.uint16
            fr = frames if frames is not None else [torch.zeros(n, dtype=dt, device=device) for _ in range(nf)]
            tabs = [torch.ones(rows * 4 + 1, dtype=torch.float64, device=device) for _ in range(3)]
            o = torch.full((3 * 6 * 4,), 7.0, dtype=torch.float64, device=device)
            w = torch.zeros(max(1, lib.hm_pairs_statistics_dn_workspace_bytes(3, 4, bits) // 8 + 1), dtype=torch.float64, device=device)
            fp = (C.c_void_p * len(fr))(*[f.data_ptr() for f in fr])
            if null_frame:
                fp[1] = None
            tp = [t.data_ptr() + table_off if use else None for t, use in zip(tabs, (icrf, diff, std))]
            lim = (C.c_double * 4)(0.1, 0.1, 0.1, 0.1), (C.c_double * 4)(0.9, 0.9, 0.9, 0.9)
            rc = lib.hm_pairs_statistics_dn(C.cast(fp, C.POINTER(C.c_void_p)), nf_, bits, tp[0], tp[1], tp[2], (C.c_int32 * 3)(*pi),
                                            (C.c_int32 * 3)(*pj), (C.c_double * 3)(0.5, 0.25, 0.5), npairs, n_, C__, lim[0] if lo else None,
                                            lim[1] if hi else None, variant, o.data_ptr() if out else None, w.data_ptr() if ws else None, stream)
            if is_cuda(device):
                torch.cuda.synchronize()
            assert bool((o == 7.0).all()) == (rc != nat.HM_OK), ("out touched on an error, or untouched on success", rc)
            return rc
        if not refusals_only:
            assert call() == nat.HM_OK and call(bits=12) == nat.HM_OK and call(std=False, diff=False) == nat.HM_OK
            assert call(bits=10, variant=1) == nat.HM_OK and call(bits=12, variant=2) == nat.HM_OK and call(variant=-1) == nat.HM_OK
            odd8 = [torch.zeros(n + 1, dtype=torch.uint8, device=device)[1:] for _ in range(nf)]
            assert call(frames=odd8) == nat.HM_OK                              # uint8 frames have no alignment rule
        for kw in (dict(n_=0), dict(n_=31), dict(C__=0), dict(C__=5, n_=30), dict(nf_=0), dict(nf_=nat.HM_MAX_FRAMES + 1), dict(npairs=0),
                   dict(lo=False), dict(hi=False), dict(icrf=False), dict(out=False), dict(ws=False), dict(bits=7), dict(bits=17),
                   dict(variant=3), dict(variant=-2), dict(diff=False), dict(null_frame=True), dict(pi=(0, 3, 1)), dict(pj=(1, -1, 2))):
            assert call(**kw) == E, kw
        assert call(table_off=4) == A
        odd16 = [torch.zeros(n + 1, dtype=torch.uint16, device=device).view(torch.uint8)[1:2 * n + 1] for _ in range(nf)]
        assert all(f.data_ptr() % 2 == 1 for f in odd16)
        assert call(bits=12, frames=odd16) == A
        assert call(bits=12, frames=odd16, pi=(0, 3, 1)) == A                 # the alignment rule comes before the pair indices
        assert call(table_off=4, bits=17) == E                                 # ... and after the depth
        assert call(bits=12, variant=1) == U and call(bits=16, variant=1, std=False, diff=False) == U
        assert call(bits=12, variant=1, pj=(1, 9, 2)) == E                     # a pair index before the table that does not fit


def check_value_errors(device):
    C_, n = 3, 30
    icrf, diff, std = tables(8, C_)
    f8 = [torch.zeros((n // C_, 1, C_), dtype=torch.uint8, device=device) for _ in range(2)]
    f16 = [torch.zeros((n // C_, 1, C_), dtype=torch.uint16, device=device) for _ in range(2)]
    pairs = [(0, 1, 0.5)]
    with backend(device):
        for frames, kw in ((f8, dict(bit_depth=8)), (f16, dict()), (f16, dict(bit_depth=8)), (f16, dict(bit_depth=17)),
                           ([f8[0], f16[0]], dict()), ([f8[0], f8[1][:5]], dict()), (f8, dict(icrf=tables(10, C_)[0])),
                           (f16, dict(bit_depth=10)), (f8, dict(std_table=std, icrf_diff=None)), (f8, dict(std_table=std[:100])),
                           (f8, dict(icrf_diff=diff[:, :2])), (f8, dict(thresholds=([0.1], [0.9]))),
                           ([f.to(torch.float64) for f in f8], dict())):
            args = dict(icrf=icrf, icrf_diff=diff, std_table=None)
            args.update(kw)
            with pytest.raises(ValueError):
                engine.pairs_statistics_dn(frames, pairs, args.pop("icrf"), **args)
        with pytest.raises(NotImplementedError):
            t12 = tables(12, C_)
            engine.pairs_statistics_dn(f16, pairs, t12[0], t12[1], t12[2], bit_depth=12, variant=1)


def make_series(device, n_images=7, shape=(64, 33, 3)):
    rng = np.random.default_rng(77)
    sets = []
    for i in range(n_images):
        dn = rng.integers(0, 256, size=shape).astype(np.uint8)
        sets.append(ImageSet(value=dn, features={"exposure": 1.0 * 1.3 ** i, "subject": "s", "illumination": "bf", "magnification": "10x"},
                             use_cupy=is_cuda(device)))
    series = ExposureSeries(input_image_sets=sets)
    series.initialize_exposure_pairs()
    assert len(series.exposure_pairs) == n_images * (n_images - 1) // 2
    return series


def check_series(device, use_std):
    """ExposureSeries.process_linearity(from_dn=True) against linearize-then-process on a deep copy; the series stays DN frames."""
    assert gs.NUM_OF_CHS == 3
    icrf, diff, std = tables(8, 3)
    series = make_series(device)
    ref = copy.deepcopy(series)
    dns = [s.measurand._dn.clone() for s in series.input_image_sets]
    series.process_linearity(icrf, 20, use_std, from_dn=True, ICRF_diff=diff, STD_data=std)
    if use_std:
        for s in ref.input_image_sets:
            s.measurand.std = s.calculate_numerical_STD(std)
    lin = ref.linearize(icrf, diff)
    lin.initialize_exposure_pairs()
    lin.process_linearity(icrf, 20, use_std)
    for got, want in zip(series.collect_exposure_pair_stats(), lin.collect_exposure_pair_stats()):
        assert got.keys() == want.keys()
        for k in got:
            if got[k].dtype == object:                                         # errors without stds: None per pair
                assert all(x is None for x in got[k].ravel()) and all(x is None for x in want[k].ravel())
            else:
                assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert any(np.isnan(s.measurand._f64().cpu().numpy()).any() for s in lin.input_image_sets)      # the default route thresholds in place
    for s, d in zip(series.input_image_sets, dns):
        m = s.measurand
        assert m._dn is not None and torch.equal(m._dn, d) and m._val is None and m._std is None


def check_series_errors(device):
    icrf, diff, std = tables(8, 3)
    series = make_series(device, 3, (8, 5, 3))
    with pytest.raises(ValueError, match="ICRF_diff and STD_data"):
        series.process_linearity(icrf, 20, True, from_dn=True, ICRF_diff=diff)
    with pytest.raises(ValueError, match="ICRF_diff and STD_data"):
        series.process_linearity(icrf, 20, True, from_dn=True, STD_data=std)
    with_std = copy.deepcopy(series)
    for s in with_std.input_image_sets:
        s.measurand.std = np.full((8, 5, 3), 0.01)
    with pytest.raises(ValueError, match="default route"):
        with_std.process_linearity(icrf, 20, True, from_dn=True, ICRF_diff=diff, STD_data=std)
    lin = series.linearize(icrf)
    lin.initialize_exposure_pairs()
    with pytest.raises(ValueError, match="from_dn measurand"):
        lin.process_linearity(icrf, 20, False, from_dn=True)
    no_pairs = make_series(device, 3, (8, 5, 3))
    no_pairs.exposure_pairs = None
    with pytest.raises(ValueError, match="own images"):
        no_pairs.process_linearity(icrf, 20, False, from_dn=True)


# ------------------------------------------------------------------------------------------------ the host build
DEV = "cpu"
STD = pytest.mark.parametrize("with_std", [False, True])


@STD
def test_parent_forms_agree(with_std):
    check_parent_forms(DEV, with_std)


@pytest.mark.parametrize("with_thr", [False, True])
@STD
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
@pytest.mark.parametrize("size", SIZES)
def test_shapes(size, C_, with_std, with_thr):
    check_shapes(DEV, size, C_, with_std, with_thr)


@STD
@pytest.mark.parametrize("n_frames,n_pairs", SHAPES)
def test_frames_pairs(n_frames, n_pairs, with_std):
    check_frames_pairs(DEV, n_frames, n_pairs, with_std)


@STD
@pytest.mark.parametrize("bits", [8, 12])
def test_alignment(bits, with_std):
    check_alignment(DEV, bits, with_std)


@pytest.mark.parametrize("bits,C_,with_std", [(8, 3, True), (10, 3, True), (12, 3, True), (12, 3, False), (12, 4, False), (16, 3, True), (16, 1, False)])
def test_depths(bits, C_, with_std):
    check_depth(DEV, bits, C_, with_std)


@pytest.mark.parametrize("bits", [8, 12])
def test_zero_std(bits):
    check_zero_std(DEV, bits)


@STD
def test_stray_bits(with_std):
    check_stray_bits(DEV, with_std)


@pytest.mark.parametrize("bits,with_std", [(8, True), (10, True), (12, True), (12, False), (16, False)])
def test_variants(bits, with_std):
    check_variants(DEV, bits, with_std)


def test_describe_device_build():
    """The device build's names, asked of the HIP library without a GPU (the entry launches nothing)."""
    for args, want in DESCRIBE:
        assert describe(nat.hip_lib, N_BIG, *args) == (nat.HM_OK, want), args
    assert describe(nat.hip_lib, N_BIG, 7, 15, 3, 1, 12, 1, 1) == (nat.HM_EUNSUPPORTED, "")
    assert describe(nat.hip_lib, N_BIG, 7, 15, 4, 0, 12, 1, 1) == (nat.HM_EUNSUPPORTED, "")
    assert describe(nat.hip_lib, N_BIG, 7, 15, 3, 0, 12, 1, 1)[0] == nat.HM_OK
    for bad in ((N_BIG + 1, 7, 15, 3, 1, 8, 0, 1), (N_BIG, 0, 15, 3, 1, 8, 0, 1), (N_BIG, 7, 0, 3, 1, 8, 0, 1), (N_BIG, 7, 15, 5, 1, 8, 0, 1),
                (N_BIG, 7, 15, 3, 1, 7, 0, 1), (N_BIG, 7, 15, 3, 1, 17, 0, 1), (N_BIG, 7, 15, 3, 1, 8, 3, 1), (N_BIG, 7, 15, 3, 1, 8, -2, 1)):
        assert describe(nat.hip_lib, *bad) == (nat.HM_EINVAL, ""), bad
    assert nat.hip_lib.hm_pairs_statistics_dn_describe(N_BIG, 7, 15, 3, 1, 8, 0, 1, None, 0) == nat.HM_EINVAL
    assert engine.pairs_statistics_dn_kernel(N_BIG, 7, 15, 3, True, 12) == "pairs_stats_dn_lds<dn=u16,bits=12,tab=global,std=1,ni=1>"


def test_describe_host_build():
    host = nat.host_lib()
    for args, _ in DESCRIBE:
        nf, npairs, C_, with_std, bits, variant, aligned = args
        want = f"host_pairs_stats_dn<dn={'u8' if bits == 8 else 'u16'},bits={bits},std={with_std}>"
        assert describe(host, N_BIG, *args) == (nat.HM_OK, want), args
    assert describe(host, N_BIG, 7, 15, 3, 1, 12, 1, 1) == (nat.HM_EUNSUPPORTED, "")
    assert describe(host, N_BIG + 1, 7, 15, 3, 1, 8, 0, 1) == (nat.HM_EINVAL, "")
    with nat.host_mode():
        assert engine.pairs_statistics_dn_kernel(N_BIG, 7, 15, 3, True, 12) == "host_pairs_stats_dn<dn=u16,bits=12,std=1>"


def test_fit_rule():
    """Table in LDS where 8 or 16 bytes x 2^bits x C + 63 KiB <= 160 KiB: 8 to 10 bits at C = 3 with stds, 12 bits value-only at C = 3."""
    for bits in range(8, 17):
        for C_ in range(1, 5):
            for with_std in (0, 1):
                fits = (16 if with_std else 8) * 2 ** bits * C_ + 63 * 1024 <= 160 * 1024
                name = describe(nat.hip_lib, N_BIG - N_BIG % 12, 7, 15, C_, with_std, bits, 0, 1)[1]
                assert f"tab={'lds' if fits else 'global'}," in name, (bits, C_, with_std, name)
                assert describe(nat.hip_lib, N_BIG - N_BIG % 12, 7, 15, C_, with_std, bits, 1, 1)[0] == (nat.HM_OK if fits else nat.HM_EUNSUPPORTED)
    assert all("tab=lds" in describe(nat.hip_lib, 12, 7, 15, 3, 1, b, 0, 1)[1] for b in (8, 9, 10))
    assert "tab=lds" in describe(nat.hip_lib, 12, 7, 15, 3, 0, 12, 0, 1)[1] and "tab=global" in describe(nat.hip_lib, 12, 7, 15, 3, 1, 12, 0, 1)[1]


def test_status_host_build():
    check_status(DEV)


def test_status_device_build_without_gpu():
    """The HIP library's refusals return before anything is launched or written, so they can be asked with host memory and no GPU: the
    same codes (check_status asserts them) from the same header."""
    check_status(DEV, lib=nat.hip_lib)


def test_symbols():
    assert nat.HM_ABI_VERSION == 2 and nat.hip_lib.hm_version() == 2 and nat.host_lib().hm_version() == 2
    for s in SYMBOLS:
        assert s in nat.EXPORTED_SYMBOLS and callable(getattr(nat.hip_lib, s)) and callable(getattr(nat.host_lib(), s))
    assert nat.hip_lib.hm_pairs_statistics_dn_workspace_bytes(15, 3, 12) >= nat.hip_lib.hm_pairs_statistics_workspace_bytes(15) + 16 * 4096 * 3


def test_value_errors():
    check_value_errors(DEV)


@STD
def test_series(with_std):
    check_series(DEV, with_std)


def test_series_errors():
    check_series_errors(DEV)


def test_series_std_file(tmp_path):
    """use_std=True without STD_data reads settings.STD_FILE_NAME, as calculate_numerical_STD(None) does."""
    icrf, diff, std = tables(8, 3)
    a, b = make_series(DEV, 3, (16, 7, 3)), make_series(DEV, 3, (16, 7, 3))
    path = tmp_path / "std.txt"
    np.savetxt(path, std)
    old = gs.STD_FILE_NAME
    try:
        gs.STD_FILE_NAME = str(path)
        a.process_linearity(icrf, 20, True, from_dn=True, ICRF_diff=diff)
    finally:
        gs.STD_FILE_NAME = old
    b.process_linearity(icrf, 20, True, from_dn=True, ICRF_diff=diff, STD_data=np.loadtxt(path))
    for x, y in zip(a.collect_exposure_pair_stats(), b.collect_exposure_pair_stats()):
        assert all(np.array_equal(x[k], y[k], equal_nan=True) for k in x)
