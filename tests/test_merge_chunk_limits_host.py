"""The chunked merge (csrc/hm_merge_chunk.hip: stacks of more than HM_MAX_FRAMES frames, or variant = -chunk on a short one) at the limits of
its ABI. The checks are functions of a device name: here they run on the HOST build (csrc_host/hm_host.cpp), which takes any number of
frames in one pass and ignores the chunking - there they pin down the cases and the oracle comparisons; tests/test_gpu_merge_chunk_limits.py
runs the same ones on the MI355X, where `variant = -chunk` goes through merge_chunk<...>.

Two criteria, the ones the kernel file documents:
    bits     every output of the call equals, bit for bit, the same call with variant = -1 (merge_generic: one launch, one element per
             thread) - a stack merged in chunks of any size gives the bits of the one-launch kernels;
    oracle   oracle/hdr_oracle.py (NumPy) at the project's VAL_RTOL / F64_RTOL / STD_RTOL, once per configuration class.
On the device `plan.kernels` must be exactly merge_chunk<f64in=..,..,hot=..,vec=..>(N=.. in chunks of ..) with the vec and hot the case
predicts: vec = 2 needs 16-byte aligned float64 arrays and 2-byte aligned byte streams AT THE TILE'S FIRST ELEMENT (the input offset
(row0 - buf_row0) W C counts), else every launch is the one-element kernel."""
import functools

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from oracle import hdr_oracle as orc

VAL_RTOL, STD_RTOL, F64_RTOL = 1e-12, 1e-9, 1e-11                           # tests/test_gpu_merge.py
MODES = ("val", "std", "S")                                                 # val only; val + std; the sum of weights alone
MODE_NAME = {"val": "val", "std": "S + std", "S": "S"}
THR = 0.5                                                                   # dark threshold; hot DNs are 210
HOST_STRIDE_E = 1_048_577


# ------------------------------------------------------------------------------------------------ plumbing
def is_cuda(device):
    return str(device).startswith("cuda")


def E(device):
    if is_cuda(device):
        return engine
    from camera_linearity_amd.measurand import _HOST_ENGINE
    return _HOST_ENGINE


def T(a, device):
    if a is None or isinstance(a, torch.Tensor):
        return a
    return torch.as_tensor(np.ascontiguousarray(a)).to(device)


def offset_view(a, device):
    """A tensor with the values of `a` that starts one element into its allocation: an odd byte for uint8, 8 but not 16 bytes for float64."""
    a = np.ascontiguousarray(a)
    big = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=device)
    big[1:] = torch.from_numpy(a).reshape(-1).to(device)
    v = big[1:].view(a.shape)
    assert v.is_contiguous() and (v.data_ptr() % 16 == 8 if a.dtype == np.float64 else v.data_ptr() % 2 == 1)
    return v


def make_icrf(c):
    icrf = np.stack([np.linspace(0, 1, 256) ** (1.6 + 0.2 * k) for k in range(c)], axis=1)
    return icrf, orc.icrf_derivative(icrf)


@functools.lru_cache(maxsize=None)
def stack(seed, n, h, w, c, f64):
    """-> (frames, stds, exposures): uint8 DNs of a radiance seen through n exposures, or those DNs / 255 with a jitter (float64)."""
    rng = np.random.default_rng(seed)
    rad = rng.random((h, w, c)) * 4
    t = 1e-3 * 1.25 ** np.arange(n)
    k = 255 / (4 * t[n // 2])
    frames = [np.clip(np.around(rad * ti * k + rng.integers(-3, 4, rad.shape)), 0, 255).astype(np.uint8) for ti in t]
    if f64:
        frames = [np.clip(orc.unit_from_u8(f) + (rng.random(f.shape) - 0.5) * 1e-3, 0.0, 1.0) for f in frames]
    stds = [0.004 * (1 + rng.random((h, w, c))) for _ in range(n)]
    return frames, stds, list(t)


def run(device, frames, t, icrf, diff, stds, mode, variant, prefill=None, **kw):
    """One merge through engine.plan_merge -> ({name: ndarray}, plan.kernels, the plan). mode: 'val' | 'std' | 'S'."""
    e = E(device)
    fr = [T(f, device) for f in frames]
    sd = [T(s, device) for s in stds] if mode == "std" else None
    kw = dict(kw)
    for key in ("flat", "flat_std"):
        if key in kw:
            kw[key] = T(kw[key], device)
    if mode != "std":
        kw.pop("flat_std", None), kw.pop("ff_std_mean", None)
    if mode == "S":
        kw.pop("flat", None), kw.pop("ff_mean", None)
    if "darks" in kw:
        kw["darks"] = [T(d, device) for d in kw["darks"]]
    plan = e.plan_merge(fr, t, icrf, diff if mode == "std" else None, sd, variant=variant, want_val=mode != "S", want_sum_w=mode == "S", **kw)
    if prefill is not None:
        prefill(plan)
    names = plan.kernels
    plan.launch()
    if is_cuda(device):
        torch.cuda.synchronize()
    assert set(plan.outputs) == {"val": {"val"}, "std": {"val", "std"}, "S": {"sum_w"}}[mode]
    return {k: v.cpu().numpy() for k, v in plan.outputs.items()}, names, plan


def kernel_name(f64, mode, hot, vec, n, chunk):
    return f"merge_chunk<f64in={int(f64)},{MODE_NAME[mode]},hot={int(hot)},vec={vec}>(N={n} in chunks of {chunk})"


def assert_names(device, names, f64, mode, hot, vec, n, chunk):
    if is_cuda(device):
        assert names == kernel_name(f64, mode, hot, vec, n, chunk), names
    else:
        assert names.startswith("merge_host<"), names


def assert_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == np.float64 and a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), f"{what}: {k} differs in {np.flatnonzero(a[k].ravel() != b[k].ravel())[:8]}"


def close(a, b, rtol, what):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=0, err_msg=what)


def assert_oracle(out, ref, mode, f64, what, flat=False):
    if mode == "S":
        return close(out["sum_w"], ref["S"], VAL_RTOL, what)
    close(out["val"], ref["val_ff" if flat else "val"], F64_RTOL if f64 else VAL_RTOL, what)
    if mode == "std":
        close(out["std"], ref["std_ff" if flat else "std"], STD_RTOL, what)


def both(device, frames, t, icrf, diff, stds, mode, chunk, f64, hot, vec, what, **kw):
    """The chunked call and the one-launch call (variant -1) of the same arguments: the same bits in every output. -> the chunked outputs."""
    a, names, _ = run(device, frames, t, icrf, diff, stds, mode, -chunk, **kw)
    assert_names(device, names, f64, mode, hot, vec, len(frames), chunk)
    b, one, _ = run(device, frames, t, icrf, diff, stds, mode, -1, **kw)
    if is_cuda(device):
        assert "merge_chunk" not in one, one
    assert_bits(a, b, what)
    return a


# ------------------------------------------------------------------------------------------------ 1: chunk boundaries
BOUNDARIES = [(6, 2), (6, 3), (6, 6), (7, 7)]           # whole chunks: `last` falls on a full one; 6 of 6 / 7 of 7: one launch, first and last
LONG = [64, 65]                                         # two full launches of 32; 32 + 32 + 1


def check_boundaries(device, n, chunk, f64, mode):
    frames, stds, t = stack(10 + n, n, 5, 7, 3, f64)
    icrf, diff = make_icrf(3)
    both(device, frames, t, icrf, diff, stds, mode, chunk, f64, False, 2, f"N={n} in chunks of {chunk}, {mode}")


def check_long(device, n, f64, mode):
    """More than HM_MAX_FRAMES frames (variant 0: chunks of 32; variant -1 is chunked too): the oracle, the bits of chunks of 5, and - uint8
    frames, where both builds perform the same IEEE operations in the same order - the bits of the host build's single pass."""
    frames, stds, t = stack(10 + n, n, 5, 7, 3, f64)
    icrf, diff = make_icrf(3)
    a, names, _ = run(device, frames, t, icrf, diff, stds, mode, 0)
    assert_names(device, names, f64, mode, False, 2, n, 32)
    ref = orc.merge(frames, t, icrf, diff if mode == "std" else None, stds=stds if mode == "std" else None)
    assert_oracle(a, ref, mode, f64, f"N={n} {mode}")
    b, names, _ = run(device, frames, t, icrf, diff, stds, mode, -5)
    assert_names(device, names, f64, mode, False, 2, n, 5)
    assert_bits(a, b, f"N={n}: chunks of 32 against chunks of 5")
    if is_cuda(device) and not f64:
        assert_bits(a, run("cpu", frames, t, icrf, diff, stds, mode, 0)[0], f"N={n}: device against the host build")


# ------------------------------------------------------------------------------------------------ 2: channel counts
CHANNEL_SHAPES = {1: (9, 13, 1), 2: (7, 9, 2), 4: (5, 5, 4)}                 # 117, 126 and 100 elements; 117, 63 and 25 pixels: odd


def check_channels(device, c, chunk, with_std, f64):
    """C = 1, 2, 4 (ch = e % C, t_g[idx * C + ch], a two-element pair that straddles a pixel) with a float64 and a uint8 flat field, and
    with frame 1 one element into its allocation (one-element kernels)."""
    h, w, _ = CHANNEL_SHAPES[c]
    n, mode = 7, "std" if with_std else "val"
    frames, stds, t = stack(40 + c, n, h, w, c, f64)
    icrf, diff = make_icrf(c)
    rng = np.random.default_rng(c)
    flat_u8 = rng.integers(170, 235, size=(h, w, c)).astype(np.uint8)
    flat_std = 0.002 * (1 + rng.random((h, w, c)))
    ffm, ffs = list(0.78 + 0.01 * np.arange(c)), [0.002] * c
    for flat in (flat_u8, orc.unit_from_u8(flat_u8) + 1e-4):
        kw = dict(flat=flat, flat_std=flat_std, ff_mean=ffm, ff_std_mean=ffs)
        what = f"C={c} chunks of {chunk} {mode} f64={f64} flat {flat.dtype}"
        a = both(device, frames, t, icrf, diff, stds, mode, chunk, f64, False, 2, what, **kw)
        fv = orc.unit_from_u8(flat) if flat.dtype == np.uint8 else flat
        if with_std:
            ref = orc.merge(frames, t, icrf, diff, stds=stds, flat=fv, flat_std=flat_std, ff_mean=np.array(ffm), ff_std_mean=np.array(ffs))
        else:
            ref = orc.merge(frames, t, icrf, None)
            ref["val_ff"] = (ref["val"] / fv) * np.array(ffm)
        assert_oracle(a, ref, mode, f64, what, flat=True)
    shifted = list(frames)
    shifted[1] = offset_view(frames[1], device)
    b = both(device, shifted, t, icrf, diff, stds, mode, chunk, f64, False, 1, f"C={c}: frame 1 offset by one element", **kw)
    assert_bits(a, b, f"C={c}: offset against aligned")


# ------------------------------------------------------------------------------------------------ 3: row tiles
H16, W37 = 16, 37                                                           # W * C = 111
# (buf_row0, buf_rows, row0, rows, median_k, vec): the input offset (row0 - buf_row0) * 111 is even -> vec 2, odd -> vec 1
ROW_TILES = [
    (3, 13, 5, 6, 3, 2), (3, 13, 5, 6, 5, 2),        # rows [5, 11): offset 222; k = 5 reaches buffer rows 3, 4 and 11, 12 outside the tile
    (3, 13, 4, 6, 3, 1),                             # rows [4, 10): offset 111; k = 3 reaches buffer row 3
    (3, 13, 9, 7, 5, 2), (3, 13, 10, 6, 5, 1),       # down to image row 15: the window reflects there (offsets 666, 777)
    (0, 13, 0, 6, 5, 2), (0, 13, 1, 6, 5, 1),        # from image row 0: the window reflects there (offsets 0, 111)
    (0, 16, 0, 16, 5, 2),                            # the whole image: both reflections in one call
]


@functools.lru_cache(maxsize=None)
def row_image(f64):
    """The 16-row image, its dark maps (None on frames 2 and 5, about 10 % hot elsewhere, rows 0, 3, 4, 11, 12 and 15 denser) and the oracle's
    merge of the whole image for k = 3 and 5."""
    n = 7
    frames, stds, t = stack(60, n, H16, W37, 3, f64)
    icrf, diff = make_icrf(3)
    rng = np.random.default_rng(61)
    darks = []
    for i in range(n):
        d = (rng.random((H16, W37, 3)) < 0.10).astype(np.uint8) * 210
        d[[0, 3, 4, 11, 12, 15]] |= (rng.random((6, W37, 3)) < 0.3).astype(np.uint8) * 210
        darks.append(None if i in (2, 5) else d)
    refs = {k: orc.merge(frames, t, icrf, diff, stds=stds, darks=[None if d is None else orc.unit_from_u8(d) for d in darks],
                         dark_threshold=THR, median_k=k) for k in (3, 5)}
    return frames, stds, t, icrf, diff, darks, refs


def check_row_tile(device, tile, f64, chunk=3):
    buf0, bufn, row0, rows, k, vec = tile
    assert ((row0 - buf0) * W37 * 3) % 2 == (0 if vec == 2 else 1)
    frames, stds, t, icrf, diff, darks, refs = row_image(f64)
    dmin = E(device).dark_min_dn(1.0, THR)
    cut = lambda a: None if a is None else a[buf0:buf0 + bufn]              # noqa: E731
    kw = dict(darks=[cut(d) for d in darks], dark_min=[256 if d is None else dmin for d in darks], median_k=k,
              height=H16, row0=row0, rows=rows, buf_row0=buf0)
    what = f"rows [{row0}, {row0 + rows}) of buffers from row {buf0}, k={k}"
    a = both(device, [cut(f) for f in frames], t, icrf, diff, [cut(s) for s in stds], "std", chunk, f64, True, vec, what, **kw)
    ref = {key: refs[k][key][row0:row0 + rows] for key in ("val", "std")}
    assert_oracle(a, ref, "std", f64, what)


# ------------------------------------------------------------------------------------------------ 4: hot-pixel placement
HOT_SHAPE = (5, 7, 3)                                                       # 105 elements: 52 pairs and an odd last element


@functools.lru_cache(maxsize=None)
def hot_maps():
    """5 frames in chunks of 2: frame 0 (where `start` and `hot` meet), frames 1 and 3 (a chunk's last frame) and 4 (the stack's last).
        frame 0   the four corners, both elements of the pair (10, 11), two adjacent pixels, the odd last element (104)
        frame 1   hot everywhere
        frame 2   no map
        frame 3   sparse, and both elements of the pair (50, 51) - which straddles two pixels
        frame 4   the four corners and the odd last element"""
    h, w, c = HOT_SHAPE
    rng = np.random.default_rng(70)
    maps = [np.zeros(HOT_SHAPE, np.uint8) for _ in range(5)]
    for m in (maps[0], maps[4]):
        m[[0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = 210
    maps[0].reshape(-1)[[10, 11]] = 210
    maps[0][2, 3] = maps[0][2, 4] = 210
    assert maps[0].reshape(-1)[104] == 210 and maps[4].reshape(-1)[104] == 210
    maps[1][:] = 255
    maps[3][rng.random(HOT_SHAPE) < 0.08] = 210
    maps[3].reshape(-1)[[50, 51]] = 210
    assert 50 // c != 51 // c
    maps[2] = None
    return maps


def check_hot_placement(device, f64, mode, k):
    h, w, c = HOT_SHAPE
    frames, stds, t = stack(71, 5, h, w, c, f64)
    icrf, diff = make_icrf(c)
    maps = hot_maps()
    dmin = E(device).dark_min_dn(1.0, THR)
    kw = dict(darks=maps, dark_min=[256 if d is None else dmin for d in maps], median_k=k)
    what = f"hot placement f64={f64} {mode} k={k}"
    a = both(device, frames, t, icrf, diff, stds, mode, 2, f64, True, 2, what, **kw)
    ref = orc.merge(frames, t, icrf, diff if mode == "std" else None, stds=stds if mode == "std" else None,
                    darks=[None if d is None else orc.unit_from_u8(d) for d in maps], dark_threshold=THR, median_k=k)
    assert_oracle(a, ref, mode, f64, what)
    # the filter did something at every placement: without the maps the outputs differ there
    plain = run(device, frames, t, icrf, diff, stds, mode, -2)[0]
    key = "sum_w" if mode == "S" else "val"
    assert (plain[key] != a[key]).reshape(-1)[[0, 10, 11, 50, 51, 104]].sum() >= 3


# ------------------------------------------------------------------------------------------------ 5: grid stride
def stride_elems(device):
    """One element more than two passes of the pair kernel's grid: 8 workgroups of 256 lanes per CU, two elements per lane."""
    if not is_cuda(device):
        return HOST_STRIDE_E
    import ctypes as C
    n, cu, lds = C.c_int(0), C.c_int(0), C.c_int(0)
    arch = C.create_string_buffer(32)
    assert nat.hip_lib.hm_device_info(C.byref(n), C.byref(cu), C.byref(lds), arch, 32) == nat.HM_OK and cu.value >= 1
    return 2 * (cu.value * 8 * 256 * 2) + 1


def check_grid_stride(device, mode):
    n_el = stride_elems(device)
    rng = np.random.default_rng(80)
    frames = [rng.integers(0, 256, size=(1, n_el, 1), dtype=np.uint8) for _ in range(3)]
    stds = [rng.random((1, n_el, 1)) * 0.02 for _ in range(3)] if mode == "std" else None
    icrf, diff = make_icrf(1)
    a = both(device, frames, [1e-3, 2e-3, 4e-3], icrf, diff, stds, mode, 2, False, False, 2, f"{n_el} elements, {mode}")
    assert np.isfinite(a["val"]).all() and (a["val"][0, -5:, 0] > 0).any() and (a["val"][0, n_el // 2:, 0] > 0).mean() > 0.5


# ------------------------------------------------------------------------------------------------ 6: the sum buffer
CANARY = 64


def check_sum_buffer(device, f64):
    """out_sum_w absent: the running sum of weights lives in frames_workspace, E * 8 bytes. Exactly that size between canaries: the bits
    of the one-launch call. 8- but not 16-byte aligned: the one-element kernels, the same bits. The device build alone needs the
    buffer: one byte short is HM_EUNSUPPORTED, 4 bytes off is HM_EALIGN, both before any launch - outputs and buffer untouched."""
    h, w, c = 5, 7, 3
    n_el = h * w * c
    frames, stds, t = stack(90, 7, h, w, c, f64)
    icrf, diff = make_icrf(c)
    want = run(device, frames, t, icrf, diff, stds, "std", -1)[0]
    raw = torch.full((n_el * 8 + 16 + 2 * CANARY,), 0xA5, dtype=torch.uint8, device=device)
    assert raw.data_ptr() % 16 == 0

    def intact(lo, size):
        r = raw.cpu().numpy()
        return bool((r[:CANARY + lo] == 0xA5).all() and (r[CANARY + lo + size:] == 0xA5).all())

    def place(lo, size):
        def prefill(plan):
            raw.fill_(0xA5)
            plan.args.frames_workspace, plan.args.frames_workspace_bytes = raw.data_ptr() + CANARY + lo, size
            for v in plan.outputs.values():
                v.view(torch.uint8).fill_(0xC3)
        return prefill

    for lo, vec in ((0, 2), (8, 1)):
        got, names, _ = run(device, frames, t, icrf, diff, stds, "std", -2, prefill=place(lo, n_el * 8))
        assert_names(device, names, f64, "std", False, vec, 7, 2)
        assert_bits(got, want, f"sum buffer at +{lo}")
        assert intact(lo, n_el * 8), "a write outside the sum buffer"
    if not is_cuda(device):
        return
    for lo, size, exc in ((0, n_el * 8 - 1, NotImplementedError), (4, n_el * 8, ValueError)):
        e = E(device)
        plan = e.plan_merge([T(f, device) for f in frames], t, icrf, diff, [T(s, device) for s in stds], variant=-2)
        place(lo, size)(plan)
        with pytest.raises(exc):
            plan.launch()
        torch.cuda.synchronize()
        assert all(bool((v.view(torch.uint8) == 0xC3).all()) for v in plan.outputs.values()), "a refused call wrote an output"
        assert bool((raw == 0xA5).all()), "a refused call wrote the sum buffer"


# ------------------------------------------------------------------------------------------------ the tests, on the host build
HOST = "cpu"
F64 = pytest.mark.parametrize("f64", [False, True], ids=["u8", "f64"])
MODE = pytest.mark.parametrize("mode", MODES)


@F64
@MODE
@pytest.mark.parametrize("n,chunk", BOUNDARIES)
def test_host_boundaries(n, chunk, f64, mode):
    check_boundaries(HOST, n, chunk, f64, mode)


@F64
@MODE
@pytest.mark.parametrize("n", LONG)
def test_host_long_stacks(n, f64, mode):
    check_long(HOST, n, f64, mode)


@F64
@pytest.mark.parametrize("with_std", [False, True])
@pytest.mark.parametrize("chunk", [2, 3])
@pytest.mark.parametrize("c", [1, 2, 4])
def test_host_channels(c, chunk, with_std, f64):
    check_channels(HOST, c, chunk, with_std, f64)


@F64
@pytest.mark.parametrize("tile", ROW_TILES)
def test_host_row_tiles(tile, f64):
    check_row_tile(HOST, tile, f64)


@F64
@pytest.mark.parametrize("mode,k", [("val", 3), ("std", 3), ("S", 3), ("std", 5), ("S", 5)])
def test_host_hot_placement(f64, mode, k):
    check_hot_placement(HOST, f64, mode, k)


@pytest.mark.parametrize("mode", ["val", "std"])
def test_host_grid_stride(mode):
    check_grid_stride(HOST, mode)


@F64
def test_host_sum_buffer(f64):
    check_sum_buffer(HOST, f64)
