"""Hot-pixel filtering in the fused merge on uint16 DN frames (hm_merge_u16_darks, engine.plan_merge(darks=[uint16 maps], bit_depth=...)),
CPU part: the host build of the C ABI, the dry dispatch and the argument rules of both libraries, and the Python surface. No GPU needed.
tests/test_gpu_merge_u16_darks.py runs the same checks (the functions below take the engine and the device) on the HIP kernels.

Three criteria; outputs are pre-filled with NaN and none may remain:
  pre-filtered  hm_merge_u16_darks(frames, darks) against hm_merge_u16(filtered) as integer bit patterns in val, std and sum_w; `filtered` is
                built here with oracle.median_filter_reflect on the masked uint16 frames and on the stds (medians of odd counts are exact).
                The result must also differ from the merge without maps in at least one element: a disabled pass cannot pass.
  embedding     a uint8 stack with uint8 maps and thresholds t, re-expressed at depth b (DN16 = DN8 << (b - 8), dark16 = dark8 << (b - 8),
                t16 = t << (b - 8); tables NaN except the embedded rows; a few elements of frames and maps carry bits above the depth) must
                give hm_merge-with-darks_u8 bits: the shift is monotonic, so medians commute.
  arithmetic    the NumPy restatement of tests/test_merge_u16_host.py on the pre-filtered frames, val 1e-12, std 1e-9 relative, atol 0.

Every case mixes its maps: one frame without a map, two frames sharing one map and threshold, one frame on that map with another threshold,
one map with threshold 2^b (nothing hot), the rest distinct. The shared map has forced hot pixels: the four corners, one on each edge, two
horizontally and two vertically adjacent ones (hot neighbours enter the median unfiltered), a dark DN equal to the threshold and one below."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import hdr_oracle as orc  # noqa: E402

import test_merge_u16_host as h16  # noqa: E402
from test_merge_u16_host import F32, F64, T, VAL_RTOL, STD_RTOL, assert_same_bits, bits_of, exposures, full_range_frames, make_stds, tables_bits  # noqa: E402

U16 = torch.uint16
SHAPES = [(13, 37, 3), (8, 64, 4), (3, 43, 1)]        # groups + a tail, odd W C; whole groups, aligned scan; H = 3 (k = 7 reflects past both edges)
BIG = (48, 456, 3)                                    # 65 664 elements: 128 past one 65 536-element scan piece
THREE_PIECES = (96, 456, 3)                           # 131 328 elements: two whole scan pieces and 256 elements of a third


def recommended_queue_entries(shape):
    """Entries of the queue in a workspace of hm_merge_hot_workspace_bytes: a quarter of the elements, but one per element for a tile of
    fewer than 4096 - the small shapes' recommended queue cannot overflow; from 16 384 elements on it holds exactly a quarter."""
    from camera_linearity_amd import _native as nat
    e = int(np.prod(shape))
    return (int(nat.hip_lib.hm_merge_hot_workspace_bytes(e)) - int(nat.hip_lib.hm_merge_hot_workspace_min_bytes(e))) // 4 + 1


def hot_count(darks, dark_min, b):
    """Elements with at least one hot frame: what the scan queues."""
    m = 2 ** b - 1
    hot = np.zeros(next(d for d in darks if d is not None).shape, dtype=bool)
    for d, t in zip(darks, dark_min):
        if d is not None:
            hot |= (d.astype(np.int64) & m) >= t
    return int(hot.sum())


def check_overflowing_recommended_queue(eng, dev, expect=None):
    """The recommended workspace really overflowing: 60 % hot per map on 65 664 elements (the first scan piece alone exceeds the 16 416
    entries), and about 30 % of 131 328 elements hot (each whole piece fits the 32 832 entries on its own, the two together do not: one
    piece is queued before the other raises the flag)."""
    for shape, n, b, k, with_std, density in ((BIG, 7, 12, 3, True, 0.6), (THREE_PIECES, 7, 16, 3, False, 0.11), (THREE_PIECES, 9, 9, 5, True, 0.09)):
        rng = np.random.default_rng(100000 * b + 1000 * n + 10 * k + shape[2])           # check_prefiltered's maps (seed = 0)
        full_range_frames(rng, n, shape, b)
        if with_std:
            make_stds(rng, n, shape)
        darks, dark_min, _ = map_mix(rng, n, shape, b, density)
        cap, count = recommended_queue_entries(shape), hot_count(darks, dark_min, b)
        assert cap == int(np.prod(shape)) // 4 and count > cap, (shape, cap, count)
        if shape == THREE_PIECES:                         # either whole piece fits on its own
            per_piece = [hot_count([None if d is None else d.reshape(-1)[lo:lo + 65536] for d in darks], dark_min, b) for lo in (0, 65536)]
            assert max(per_piece) < cap < sum(per_piece), (per_piece, cap)
        check_prefiltered(eng, dev, shape, n, b, k, with_std, density=density, workspace="rec", expect=expect)
DEPTHS = [9, 12, 16]


@pytest.fixture()
def heng():
    from camera_linearity_amd.measurand import _HOST_ENGINE
    return _HOST_ENGINE


def high_bits(b):
    return np.uint16((0xFFFF << b) & 0xFFFF)


def thresholds(b):
    """(the shared map's threshold, the other threshold on the same map, 'nothing hot')."""
    return 3 << (b - 2), 1 << (b - 1), 1 << b


def forced_positions(h, w):
    """(row, col): corners, one on each edge, two horizontally adjacent, two vertically adjacent."""
    return [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 2, w - 1),
            (1, 5), (1, 6), (0, 10), (1, 10)]


def random_map(rng, shape, b, density, thr, thr_low):
    """Dark DNs below thr_low (hot under no threshold), a share `density` at or above thr, a few between the two thresholds; below 16 bits
    a few elements carry bits above the depth (a map read unmasked would call them hot)."""
    d = rng.integers(0, thr_low - 1, size=shape).astype(np.uint16)
    hot = rng.random(shape) < density
    d[hot] = rng.integers(thr, 1 << b, size=int(hot.sum())).astype(np.uint16)
    flat = d.reshape(-1)
    flat[rng.choice(flat.size, size=min(7, flat.size), replace=False)] = rng.integers(thr_low, thr, size=min(7, flat.size)).astype(np.uint16)
    if b < 16:
        flat[rng.choice(flat.size, size=min(9, flat.size), replace=False)] |= high_bits(b)
    return d


def map_mix(rng, n, shape, b, density):
    """-> (darks: N arrays or None, dark_min: N ints, distinct: number of distinct (map, threshold) pairs)."""
    h, w, c = shape
    t_a, t_low, t_none = thresholds(b)
    a = random_map(rng, shape, b, density, t_a, t_low)
    for j, (r, x) in enumerate(forced_positions(h, w)):
        a[r, x, j % c] = t_a + (j % 3)                                   # (position 0: exactly the threshold)
    a[1, 20, 0] = t_a                                                    # equal to the threshold: hot
    a[1, 22, 0] = t_a - 1                                                # one below: not hot for t_a (hot for the lower threshold)
    if a.size > 65536:
        a.reshape(-1)[65535] = a.reshape(-1)[65536] = t_a + 1            # the last element of the first scan piece, the first of the second
    if n == 1:
        return [a], [t_a], 1
    roles = [None, ("a", t_a), ("a", t_a), ("a", t_low), ("b", t_none)] + [(f"d{i}", t_a) for i in range(5, n)]
    maps = {"a": a, "b": random_map(rng, shape, b, density, t_a, t_low)}
    darks, dark_min = [], []
    for role in roles[:n]:
        if role is None:
            darks.append(None)
            dark_min.append(t_none)
            continue
        key, thr = role
        if key not in maps:
            maps[key] = random_map(rng, shape, b, density, t_a, t_low)
        darks.append(maps[key])
        dark_min.append(thr)
    return darks, dark_min, len({(id(d), t) for d, t in zip(darks, dark_min) if d is not None})


def prefilter(frames, stds, darks, dark_min, b, k):
    """The reference's pass (measurand.py:543-557) on masked DNs: where (dark & M) >= threshold the k x k median of the frame / of the std."""
    m = np.uint16(2 ** b - 1)
    out_f, out_s = [], []
    for i, f in enumerate(frames):
        fm = f & m
        s = None if stds is None else stds[i]
        if darks[i] is not None:
            hot = (darks[i] & m).astype(np.int64) >= dark_min[i]
            fm = np.where(hot, orc.median_filter_reflect(fm, k), fm)
            if s is not None:
                s = np.where(hot, orc.median_filter_reflect(s, k), s)
        out_f.append(fm)
        out_s.append(s)
    return out_f, (None if stds is None else out_s)


def up(x, dev):
    return None if x is None else T(x, dev)


def set_workspace(plan, workspace):
    """'rec': the recommended workspace plan_merge allocated; 'min': the same buffer declared with the smallest legal size (one entry)."""
    from camera_linearity_amd import _native as nat
    if workspace == "min":
        e = plan.args.rows * plan.args.width * plan.args.channels
        plan.args.hot_workspace_bytes = int(nat.hip_lib.hm_merge_hot_workspace_min_bytes(e))
        assert plan.args.hot_workspace and plan.args.hot_workspace_bytes < int(nat.hip_lib.hm_merge_hot_workspace_bytes(e))


def run_nan_filled(plan):
    for o in plan.outputs.values():
        o.fill_(float("nan"))
    plan.launch()
    return plan.outputs


def check_prefiltered(eng, dev, shape, n, b, k, with_std, density=0.01, workspace="rec", variants=(0,), tile=None, with_flat=False, seed=0,
                      expect=None, **kw):
    """Criterion 1 -> {variant: plan.kernels}. tile = (height, row0, rows, buf_row0): `shape` is the whole image, the buffers cover rows
    [buf_row0, height)."""
    h, w, c = shape
    rng = np.random.default_rng(100000 * b + 1000 * n + 10 * k + c + seed)
    frames = full_range_frames(rng, n, shape, b)
    stds = make_stds(rng, n, shape) if with_std else None
    darks, dark_min, _ = map_mix(rng, n, shape, b, density)
    filt_f, filt_s = prefilter(frames, stds, darks, dark_min, b, k)
    icrf, diff = tables_bits(c, b)
    t = exposures(n)
    geo, rows, cut = {}, h, slice(None)
    if tile is not None:
        height, row0, rows, buf_row0 = tile
        assert h == height
        geo, cut = dict(height=height, row0=row0, rows=rows, buf_row0=buf_row0), slice(buf_row0, None)
    if with_flat:
        kw.update(h16.flat_kw(rng, rows, w, c, with_std))
    kw = {key: (T(v, dev) if isinstance(v, np.ndarray) else v) for key, v in kw.items()}

    def sl(xs):
        """The buffers' rows of every array on the device; one tensor per distinct array (frames that share a map share its pointer)."""
        seen = {}
        return None if xs is None else [None if x is None else seen.setdefault(id(x), T(x[cut], dev)) for x in xs]
    names = {}
    for v in variants:
        common = dict(bit_depth=b, variant=v, **geo, **kw)
        want = run_nan_filled(eng.plan_merge(sl(filt_f), t, icrf, diff if with_std else None, sl(filt_s), **common))
        plain = run_nan_filled(eng.plan_merge(sl(frames), t, icrf, diff if with_std else None, sl(stds), **common))
        plan = eng.plan_merge(sl(frames), t, icrf, diff if with_std else None, sl(stds), darks=sl(darks), dark_min=dark_min, median_k=k,
                              hot_queue=workspace != "none", **common)
        assert plan._entry == "hm_merge_u16_darks"
        set_workspace(plan, workspace)
        got = run_nan_filled(plan)
        assert got.keys() == want.keys()
        for key in want:
            assert_same_bits(got[key], want[key], f"{key} b={b} k={k} variant={v} {workspace} {plan.kernels}")
        assert any(not np.array_equal(bits_of(got[key]), bits_of(plain[key])) for key in want), "the pass changed nothing"
        names[v] = plan.kernels
        if expect is not None:
            expect(v, names[v], workspace)
    return names


def check_embedding(eng, dev, shape, n, b, k, with_std, workspace="rec", seed=0, **kw):
    """Criterion 2: against hm_merge with darks_u8 on the uint8 stack."""
    from camera_linearity_amd import engine
    h, w, c = shape
    rng = np.random.default_rng(5000 * b + 10 * n + k + c + seed)
    f8 = [rng.integers(0, 256, size=shape).astype(np.uint8) for _ in range(n)]
    d16, min16, _ = map_mix(rng, n, shape, 16, 0.02)
    d8 = [None if d is None else (d >> 8).astype(np.uint8) for d in d16]               # the mix's structure at 8 bits
    min8 = [t >> 8 for t in min16]                                                      # 192, 128, 256
    f16 = [f.astype(np.uint16) << (b - 8) for f in f8]
    e16 = [None if d is None else d.astype(np.uint16) << (b - 8) for d in d8]
    if b < 16:
        for x in f16 + [d for d in e16 if d is not None]:
            x.reshape(-1)[rng.choice(x.size, size=min(5, x.size), replace=False)] |= high_bits(b)
    icrf8, diff8 = h16.tables8(c)
    sd = [T(s, dev) for s in make_stds(rng, n, shape)] if with_std else None
    t = exposures(n)
    kw = {key: (T(v, dev) if isinstance(v, np.ndarray) else v) for key, v in kw.items()}
    hq = workspace != "none"
    ref = eng.plan_merge([T(f, dev) for f in f8], t, icrf8, diff8 if with_std else None, sd, darks=[up(d, dev) for d in d8], dark_min=min8,
                         median_k=k, hot_queue=hq, **kw)
    ref.launch()
    w8, dw8 = engine.weight_luts_host()
    plan = eng.plan_merge([T(f, dev) for f in f16], t, h16.embed_table(icrf8, b), h16.embed_table(diff8, b) if with_std else None, sd,
                          darks=[up(d, dev) for d in e16], dark_min=[m << (b - 8) for m in min8], median_k=k, hot_queue=hq, bit_depth=b, **kw)
    h16.swap_weight_tables(plan, T(h16.embed_table(w8, b), dev), T(h16.embed_table(dw8, b), dev))
    set_workspace(plan, workspace)
    got = run_nan_filled(plan)
    assert got.keys() == ref.outputs.keys()
    for key in got:
        assert_same_bits(got[key], ref.outputs[key], f"{key} b={b} k={k} {plan.kernels}")
    return plan.kernels


def check_arithmetic(eng, dev, shape, n, b, k, with_std, with_flat=False, workspace="rec"):
    """Criterion 3: full-range DNs, the NumPy restatement on the pre-filtered frames."""
    h, w, c = shape
    rng = np.random.default_rng(9000 + 100 * b + n + c + k)
    frames = full_range_frames(rng, n, shape, b)
    stds = make_stds(rng, n, shape) if with_std else None
    darks, dark_min, _ = map_mix(rng, n, shape, b, 0.02)
    filt_f, filt_s = prefilter(frames, stds, darks, dark_min, b, k)
    icrf, diff = tables_bits(c, b)
    t = exposures(n)
    kw = h16.flat_kw(rng, h, w, c, with_std) if with_flat else {}
    want = h16.numpy_merge_u16(filt_f, b, t, icrf, diff, filt_s, **kw)
    got = eng.merge([T(f, dev) for f in frames], t, icrf, diff if with_std else None, None if stds is None else [T(s, dev) for s in stds],
                    darks=[up(d, dev) for d in darks], dark_min=dark_min, median_k=k, hot_queue=workspace != "none", bit_depth=b, want_sum_w=True,
                    **{key: (T(v, dev) if isinstance(v, np.ndarray) else v) for key, v in kw.items()})
    np.testing.assert_allclose(got["val"].cpu().numpy(), want["val"], rtol=VAL_RTOL, atol=0)
    np.testing.assert_allclose(got["sum_w"].cpu().numpy(), want["sum_w"], rtol=VAL_RTOL, atol=0)
    if with_std:
        np.testing.assert_allclose(got["std"].cpu().numpy(), want["std"], rtol=STD_RTOL, atol=0)


def check_relaunch(eng, dev, launch_again=None):
    """A plan launched, its dark maps overwritten in place with another pattern, launched again: the second result is criterion 1 for the
    new maps - the second launch reads the maps again and nothing of the first result survives. launch_again(plan): how the second launch
    is made (default plan.launch()). This cannot show a missing reset of the queue's counters: the patch kernel forms every queued
    element's hot mask from the maps again, so a stale entry is recomputed to its plain value and a stale count only selects the
    every-element form. That the counters are zeroed before the scan (memory safety: the workspace is uninitialised) rests on the code."""
    shape, n, b, k = (13, 37, 3), 7, 12, 3
    rng = np.random.default_rng(77)
    frames = full_range_frames(rng, n, shape, b)
    stds = make_stds(rng, n, shape)
    icrf, diff = tables_bits(3, b)
    t = exposures(n)
    darks, dark_min, _ = map_mix(rng, n, shape, b, 0.3)
    dev_darks = [None if d is None else T(d.copy(), dev) for d in darks]      # one buffer per frame: each is overwritten on its own
    plan = eng.plan_merge([T(f, dev) for f in frames], t, icrf, diff, [T(s, dev) for s in stds], darks=dev_darks, dark_min=dark_min, median_k=k,
                          bit_depth=b, want_sum_w=True)
    first = {key: o.clone() for key, o in run_nan_filled(plan).items()}
    new, _, _ = map_mix(np.random.default_rng(78), n, shape, b, 0.002)
    for d, x in zip(dev_darks, new):
        if d is not None:
            d.copy_(T(x, dev))
    for o in plan.outputs.values():
        o.fill_(float("nan"))
    (launch_again or (lambda p: p.launch()))(plan)
    for pattern, got in ((darks, first), (new, plan.outputs)):
        filt_f, filt_s = prefilter(frames, stds, pattern, dark_min, b, k)
        want = eng.merge([T(f, dev) for f in filt_f], t, icrf, diff, [T(s, dev) for s in filt_s], bit_depth=b, want_sum_w=True)
        for key in want:
            assert_same_bits(got[key], want[key], key)
    assert not np.array_equal(bits_of(first["val"]), bits_of(plan.outputs["val"]))


# ---------------------------------------------------------------------------------------------- host build
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("b", DEPTHS)
def test_host_prefiltered(heng, shape, b):
    for n, k, with_std in ((7, 3, False), (9, 5, True), (7, 7, True)):
        names = check_prefiltered(heng, None, shape, n, b, k, with_std)
        assert names[0].startswith("merge_u16_host<") and f"bits={b}" in names[0] and f"hot={k}" in names[0]
    check_prefiltered(heng, None, shape, 7, b, 3, True, with_flat=True, want_sum_w=True, out_dtype=F32)
    check_prefiltered(heng, None, shape, 9, b, 3, False, with_flat=True, density=0.6)
    check_prefiltered(heng, None, shape, 7, b, 3, False, want_val=False, want_sum_w=True)          # the sum-of-weights-only call


@pytest.mark.parametrize("n", [1, 32])
def test_host_frame_counts(heng, n):
    check_prefiltered(heng, None, (13, 37, 3), n, 12, 3, True, want_sum_w=True)
    check_prefiltered(heng, None, (13, 37, 3), n, 9, 5, False)


def test_host_two_scan_pieces(heng):
    check_prefiltered(heng, None, BIG, 7, 12, 3, True)


def test_host_cases_that_overflow_the_recommended_queue(heng):
    check_overflowing_recommended_queue(heng, None)


@pytest.mark.parametrize("tile", [(16, 5, 6, 3), (16, 4, 6, 3), (16, 0, 5, 0), (16, 11, 5, 9)], ids=["even-offset", "odd-offset", "top", "bottom"])
def test_host_row_tiles(heng, tile):
    for with_std in (False, True):
        check_prefiltered(heng, None, (16, 37, 3), 7, 12, 3, with_std, tile=tile, with_flat=True)
    if tile[1] > 3:
        check_prefiltered(heng, None, (16, 37, 3), 7, 12, 5, True, tile=(tile[0], tile[1], tile[2], tile[1] - 2))      # k = 5: two halo rows


@pytest.mark.parametrize("b", DEPTHS)
def test_host_embedding(heng, b):
    rng = np.random.default_rng(b)
    for shape, n, k, with_std in (((13, 37, 3), 7, 3, True), ((8, 64, 4), 9, 5, False), ((3, 43, 1), 7, 7, True)):
        h, w, c = shape
        check_embedding(heng, None, shape, n, b, k, with_std, want_sum_w=True)
        check_embedding(heng, None, shape, n, b, k, with_std, out_dtype=F32, **h16.flat_kw(rng, h, w, c, with_std))


@pytest.mark.parametrize("b", DEPTHS)
def test_host_arithmetic(heng, b):
    check_arithmetic(heng, None, (13, 37, 3), 7, b, 3, with_std=True)
    check_arithmetic(heng, None, (8, 64, 4), 9, b, 5, with_std=False, with_flat=True)
    check_arithmetic(heng, None, (3, 43, 1), 2, b, 7, with_std=True, with_flat=True)


def test_host_relaunch(heng):
    check_relaunch(heng, None)


# ---------------------------------------------------------------------------------------------- dispatch and rules (both libraries, dry)
BASE = h16.BASE
_args, _frames = h16._args, h16._frames


def _darks(n=7, offset=0, which=None):
    """Fake dark map pointers: `which` = indices that have a map (default: all), every map distinct."""
    which = range(n) if which is None else which
    return (C.c_void_p * n)(*[(BASE * (100 + i) + offset if i in which else None) for i in range(n)])


def _hot_args(n=7, median_k=3, dark_min=None, ws=False, **kw):
    a = _args(n=n, **kw)
    dm = (C.c_int32 * n)(*([1000] * n if dark_min is None else dark_min))
    a.dark_min_dn, a.median_k = C.cast(dm, C.POINTER(C.c_int32)), median_k
    a._keep.append(dm)
    if ws:
        a.hot_workspace, a.hot_workspace_bytes = BASE * 200, 1 << 24
    return a


def _describe(lib, a, fr, dk, bits):
    buf = C.create_string_buffer(1024)
    rc = lib.hm_merge_u16_darks_describe(C.byref(a), fr, dk, bits, C.addressof(buf), 1024)
    return rc, buf.value.decode()


def test_describe_names_scan_and_patch_exactly_when_a_map_is_present():
    from camera_linearity_amd import _native as nat
    lib = nat.hip_lib
    for kw, bits in ((dict(), 12), (dict(std=True), 12), (dict(H=13, W=37), 9), (dict(variant=-1, std=True, out_kind=1), 16), (dict(sumw=True, flat=True), 14)):
        plain = h16._describe(lib, _args(**kw), _frames(), bits)
        assert plain[0] == nat.HM_OK
        std = int(bool(kw.get("std")))
        f32 = ",out=f32" if kw.get("out_kind") else ""
        for k in (3, 5, 7):
            rc, got = _describe(lib, _hot_args(median_k=k, dark_min=[100] * 7, ws=True, **kw), _frames(), _darks(which=[2]), bits)
            assert rc == nat.HM_OK and got == f"{plain[1]} + merge_u16_scan_hot + merge_u16_patch_hot<bits={bits},std={std},k={k}{f32}>", got
            rc, got = _describe(lib, _hot_args(median_k=k, dark_min=[100] * 7, **kw), _frames(), _darks(), bits)
            assert rc == nat.HM_OK and got == f"{plain[1]} + merge_u16_patch_hot<bits={bits},std={std},k={k},queue=0{f32}>", got
        # a workspace that is too small or not 16-byte aligned: the workspace-free form
        for nbytes, addr in ((16, BASE * 200), (1 << 24, BASE * 200 + 8)):
            a = _hot_args(dark_min=[100] * 7, ws=True, **kw)
            a.hot_workspace, a.hot_workspace_bytes = addr, nbytes
            assert "queue=0" in _describe(lib, a, _frames(), _darks(), bits)[1]
        # every entry NULL: hm_merge_u16's string, whatever median_k and the thresholds say
        for x in (lib, nat.host_lib()):
            rc, got = _describe(x, _hot_args(median_k=4, dark_min=[0] * 7, ws=True, **kw), _frames(), _darks(which=[]), bits)
            assert (rc, got) == h16._describe(x, _args(**kw), _frames(), bits) and rc == nat.HM_OK
        rc, got = _describe(nat.host_lib(), _hot_args(median_k=5, dark_min=[100] * 7, **kw), _frames(), _darks(), bits)
        assert rc == nat.HM_OK and got.startswith("merge_u16_host<") and "hot=5" in got


def test_abi_unchanged_and_symbols():
    from camera_linearity_amd import _native as nat
    assert C.sizeof(nat.MergeArgs) == 296 and nat.hip_lib.hm_version() == 2 and nat.host_lib().hm_version() == 2
    for name in ("hm_merge_u16_darks", "hm_merge_u16_darks_describe", "hm_merge_u16_darks_algorithmic_bytes"):
        assert name in nat.EXPORTED_SYMBOLS
        for lib in (nat.hip_lib, nat.host_lib()):
            assert callable(getattr(lib, name))


def test_algorithmic_bytes():
    """hm_merge_u16's count plus 2 bytes per element for every distinct (map, threshold)."""
    from camera_linearity_amd import _native as nat
    n, E = 7, 64 * 64 * 3
    for kw in (dict(), dict(std=True, flat=True, sumw=True)):
        for lib in (nat.hip_lib, nat.host_lib()):
            base = lib.hm_merge_u16_algorithmic_bytes(C.byref(_args(**kw)))
            count = lambda dk, dm: lib.hm_merge_u16_darks_algorithmic_bytes(C.byref(_hot_args(dark_min=dm, **kw)), dk) - base   # noqa: E731
            assert count(_darks(), [1000] * n) == 2 * n * E                                     # all distinct
            assert count(_darks(which=[]), [1000] * n) == 0 and count(None, [1000] * n) == 0
            shared = (C.c_void_p * n)(*([None] + [BASE * 100] * 3 + [BASE * 101] * 3))
            assert count(shared, [1000] * n) == 2 * 2 * E                                       # two maps, one threshold each
            assert count(shared, [1000, 1000, 1000, 500, 4096, 4096, 1000]) == 2 * 4 * E        # (a, 1000) (a, 500) (b, 4096) (b, 1000)
    assert nat.hip_lib.hm_merge_u16_darks_algorithmic_bytes(None, None) == 0


@pytest.mark.parametrize("which", ["hip", "host"])
def test_status_codes(which):
    """Every new refusal in its documented order, and hm_merge_u16's rules unchanged through the new entry."""
    from camera_linearity_amd import _native as nat
    lib = nat.hip_lib if which == "hip" else nat.host_lib()
    buf = C.create_string_buffer(256)

    def rc(a, fr=None, dk=0, n=7, offset=0, doff=0, bits=12):
        return lib.hm_merge_u16_darks_describe(C.byref(a), _frames(n, offset) if fr is None else fr, _darks(n, doff) if dk == 0 else dk, bits,
                                               C.addressof(buf), 256)
    assert rc(_hot_args()) == nat.HM_OK
    # 1. HM_EINVAL: hm_merge_u16's first group, then the entry's own - all before the alignment rules
    assert lib.hm_merge_u16_darks(None, 8, 8, 12, None) == nat.HM_EINVAL
    assert lib.hm_merge_u16_darks_describe(None, 8, 8, 12, C.addressof(buf), 256) == nat.HM_EINVAL
    assert rc(_hot_args(struct_size=100), offset=1) == nat.HM_EINVAL
    a = _hot_args()
    fr = _frames()
    a.frames_u8 = C.cast(fr, C.POINTER(C.c_void_p))
    assert rc(a, offset=1) == nat.HM_EINVAL
    assert lib.hm_merge_u16_darks_describe(C.byref(_hot_args()), None, _darks(), 12, C.addressof(buf), 256) == nat.HM_EINVAL
    for bits in (8, 17):
        assert rc(_hot_args(), offset=1, bits=bits) == nat.HM_EINVAL
    a = _hot_args(std=True)
    a.dw_lut = None
    assert rc(a, offset=1) == nat.HM_EINVAL
    assert rc(_hot_args(), dk=None, offset=1) == nat.HM_EINVAL                       # NULL darks_u16
    assert lib.hm_merge_u16_darks(C.byref(_hot_args()), _frames(), None, 12, None) == nat.HM_EINVAL
    a = _hot_args()
    d8 = _darks()
    a.darks_u8 = C.cast(d8, C.POINTER(C.c_void_p))
    assert rc(a, offset=1) == nat.HM_EINVAL                                           # darks_u8 beside the uint16 maps
    assert rc(_args(), offset=1, doff=1) == nat.HM_EINVAL                             # no dark_min_dn
    assert rc(_args(), dk=_darks(which=[])) == nat.HM_EINVAL                          # ... even when every entry is NULL
    # 2. HM_EALIGN: frames, then maps; before every remaining rule
    assert rc(_hot_args(), offset=1) == nat.HM_EALIGN
    assert rc(_hot_args(), doff=1) == nat.HM_EALIGN
    assert lib.hm_merge_u16_darks(C.byref(_hot_args()), _frames(), _darks(7, 1), 12, None) == nat.HM_EALIGN
    a = _hot_args(median_k=4)
    a.exposures = None
    assert rc(a, doff=1) == nat.HM_EALIGN
    assert rc(_hot_args(), doff=2) == nat.HM_OK                                       # 2-byte aligned maps are legal (the scalar scan)
    # 3. hm_merge's rules with the hot-pixel checks in their place
    assert rc(a) == nat.HM_EINVAL                                                     # no exposures
    assert rc(_hot_args(C_=5)) == nat.HM_EUNSUPPORTED
    assert rc(_hot_args(H=8, row0=4, buf_row0=5)) == nat.HM_ESHAPE
    for k in (0, 1, 2, 4, 6, 8, 9):
        assert rc(_hot_args(median_k=k, dark_min=[0] * 7, H=16, row0=5, buf_row0=5)) == nat.HM_EINVAL, k      # before the halo and the thresholds
    for k in (3, 5, 7):
        r = k // 2
        assert rc(_hot_args(median_k=k, H=16, row0=5, buf_row0=5 - r)) == nat.HM_OK
        assert rc(_hot_args(median_k=k, dark_min=[0] * 7, H=16, row0=5, buf_row0=6 - r)) == nat.HM_ESHAPE     # one halo row short: before the thresholds
        assert rc(_hot_args(median_k=k, H=16, row0=0, buf_row0=0)) == nat.HM_OK                              # the image edge needs no halo
        a = _hot_args(median_k=k, H=16)
        a.rows, a.buf_rows = 8, 8 + r - 1                                             # rows [0, 8) from a buffer one row short below
        assert rc(a) == nat.HM_ESHAPE
        a.buf_rows = 8 + r
        assert rc(a) == nat.HM_OK
    for bits in (9, 12, 16):
        top = 1 << bits
        assert rc(_hot_args(dark_min=[top] * 7), bits=bits) == nat.HM_OK and rc(_hot_args(dark_min=[1] * 7), bits=bits) == nat.HM_OK
        for bad in (0, -1, top + 1):
            assert rc(_hot_args(dark_min=[5, 5, bad, 5, 5, 5, 5]), bits=bits) == nat.HM_EINVAL, (bits, bad)
            assert rc(_hot_args(dark_min=[5, 5, bad, 5, 5, 5, 5]), dk=_darks(which=[0, 1, 3]), bits=bits) == nat.HM_OK   # a frame without a map
        assert rc(_hot_args(dark_min=[0] * 7, variant=4), bits=bits) == nat.HM_EINVAL
    a = _hot_args()
    a.out_val = BASE * 42 + 4
    assert rc(a) == nat.HM_EALIGN
    assert rc(_hot_args(variant=4)) == nat.HM_EINVAL and rc(_hot_args(variant=3)) == nat.HM_OK
    a = _hot_args(sumw=True)                                                          # sum of weights only
    a.out_val = None
    assert rc(a) == nat.HM_OK
    # 4. HM_EUNSUPPORTED: hm_merge_u16's
    a = _hot_args()
    a.flat_u8 = BASE * 46
    assert rc(a) == nat.HM_EUNSUPPORTED
    assert rc(_hot_args(n=33), n=33) == nat.HM_EUNSUPPORTED
    assert rc(_hot_args(variant=-2)) == nat.HM_EUNSUPPORTED
    assert rc(_hot_args(variant=1), bits=13) == nat.HM_EUNSUPPORTED and rc(_hot_args(variant=1), bits=12) == nat.HM_OK
    # hm_merge_u16 itself keeps refusing darks_u8
    a = _hot_args()
    a.darks_u8 = C.cast(d8, C.POINTER(C.c_void_p))
    assert lib.hm_merge_u16_describe(C.byref(a), _frames(), 12, C.addressof(buf), 256) == nat.HM_EUNSUPPORTED


# ---------------------------------------------------------------------------------------------- Python surface
@pytest.mark.parametrize("b", DEPTHS)
def test_dark_min_dn_with_a_depth(b):
    from camera_linearity_amd import engine
    dn = np.arange(2 ** b, dtype=np.float64)
    for scale, thr in ((1.0, 0.05), (0.37, 0.1), (2.5, 0.9), (1.0, 0.0), (0.5, 0.6), (1.0, 1.0), (3.0, 2.999)):
        v = dn / (2 ** b - 1)
        if scale != 1.0:
            v = scale * v
        hot = np.nonzero(v > thr)[0]
        assert engine.dark_min_dn(scale, thr, bit_depth=b) == (int(hot[0]) if hot.size else 2 ** b), (scale, thr)
    assert engine.dark_min_dn(0.5, 0.6, b) == 2 ** b
    for bad in (8, 17, 12.0, True):
        with pytest.raises(ValueError, match="bit_depth"):
            engine.dark_min_dn(1.0, 0.05, bit_depth=bad)


def test_dark_min_dn_default_unchanged():
    from camera_linearity_amd import engine
    for scale, thr in ((1.0, 0.05), (0.37, 0.1), (1.0, 0.0), (0.5, 0.6)):
        v = np.arange(256, dtype=np.uint8).astype(np.float64) / 255
        if scale != 1.0:
            v = np.array([scale]) * v
        hot = np.nonzero(v > thr)[0]
        assert engine.dark_min_dn(scale, thr) == (int(hot[0]) if hot.size else 256) == engine.dark_min_dn(scale, thr, None)
    assert engine.dark_min_dn(1.0, 0.05) == 13


def test_plan_merge_rules(heng):
    from camera_linearity_amd import _native as nat
    rng = np.random.default_rng(3)
    n, shape, b = 3, (6, 37, 3), 12
    f16 = [T(f) for f in full_range_frames(rng, n, shape, b)]
    f8 = [T(rng.integers(0, 256, size=shape).astype(np.uint8)) for _ in range(n)]
    d16 = T(rng.integers(0, 4096, size=shape).astype(np.uint16))
    t = exposures(n)
    icrf, diff = tables_bits(3, b)
    for bad in (f8[0], f8[0].double(), f8[0].to(torch.int16), f8[0].float()):              # uint8 and other dtypes: pinned, now naming uint16
        with pytest.raises(NotImplementedError, match="dark.*uint16|uint16.*dark"):
            heng.plan_merge(f16, t, icrf, darks=[None, bad, None], dark_min=[4096, 3, 4096], bit_depth=b)
    with pytest.raises(ValueError, match="uint16"):
        heng.plan_merge(f16, t, icrf, darks=[None, d16[:5], None], dark_min=[4096, 3, 4096], bit_depth=b)       # shape
    with pytest.raises(ValueError, match="uint8"):
        heng.plan_merge(f8, t, h16.tables8(3)[0], darks=[None, d16, None], dark_min=[256, 3, 256])              # uint16 maps with uint8 frames
    with pytest.raises(ValueError, match="one entry per frame"):
        heng.plan_merge(f16, t, icrf, darks=[None, d16], dark_min=[4096, 3], bit_depth=b)
    with pytest.raises(ValueError, match="one entry per frame"):
        heng.plan_merge(f16, t, icrf, darks=[None, d16, None], bit_depth=b)
    for bad_min in ([4096, 0, 4096], [4096, 4097, 4096]):
        with pytest.raises(ValueError):
            heng.plan_merge(f16, t, icrf, darks=[None, d16, None], dark_min=bad_min, bit_depth=b)
    with pytest.raises(ValueError):
        heng.plan_merge(f16, t, icrf, darks=[None, d16, None], dark_min=[4096, 3000, 4096], median_k=4, bit_depth=b)
    with pytest.raises(ValueError):                                                         # a row tile without its halo
        heng.plan_merge(f16, t, icrf, darks=[None, d16, None], dark_min=[4096, 3000, 4096], bit_depth=b, height=10, row0=2, buf_row0=2)
    # all-None maps: hm_merge_u16 as ever
    p = heng.plan_merge(f16, t, icrf, darks=[None] * n, dark_min=[1] * n, bit_depth=b)
    assert p._entry == "hm_merge_u16" and "hot" not in p.kernels
    # a plan with maps goes through hm_merge_u16_darks, with the workspace allocated as for 8-bit frames
    lib = nat.host_lib()
    calls = lib.calls["hm_merge_u16_darks"]
    E = int(np.prod(shape))
    p = heng.plan_merge(f16, t, icrf, darks=[None, d16, d16], dark_min=[4096, 3000, 3000], bit_depth=b)
    assert p._entry == "hm_merge_u16_darks" and not p.args.darks_u8 and p.args.median_k == 3
    assert p.args.hot_workspace and p.args.hot_workspace_bytes == lib.hm_merge_hot_workspace_bytes(E)
    assert p.algorithmic_bytes == (2 * n + 8 + 2) * E
    p.launch()
    assert lib.calls["hm_merge_u16_darks"] == calls + 1
    p = heng.plan_merge(f16, t, icrf, darks=[None, d16, d16], dark_min=[4096, 3000, 2000], bit_depth=b, hot_queue=False)
    assert not p.args.hot_workspace and p.algorithmic_bytes == (2 * n + 8 + 4) * E
    # engine.sum_of_weights follows
    S, S2 = heng.sum_of_weights(f16, darks=[None, d16, d16], dark_min=[4096, 3000, 3000], bit_depth=b)
    filt, _ = prefilter([f.numpy() for f in f16], None, [None, d16.numpy(), d16.numpy()], [4096, 3000, 3000], b, 3)
    want = heng.plan_merge([T(f) for f in filt], t, icrf, bit_depth=b, want_sum_w=True, want_val=False)
    want.launch()
    assert_same_bits(S, want.outputs["sum_w"], "sum_of_weights")
    assert S.dtype == F64 and np.array_equal(S2.numpy(), S.numpy() * S.numpy())
