"""float32 outputs of the fused merge (hm_merge_args.out_kind = HM_OUT_F32, engine.plan_merge(out_dtype=torch.float32)), CPU part: the host
build of the C ABI and the dry dispatch (hm_merge_describe) of the HIP library. No GPU needed.

The criterion is exact: all arithmetic stays float64 and the result is rounded once, to nearest even, at the store - so for the same inputs
the float32 output equals the NumPy conversion of the float64 output of the same call: NaNs at the same positions, every other element
bit-identical as int32 (signed zeros, infinities and float32 subnormals included). sum_w stays float64 and is bit-identical."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import hdr_oracle as orc  # noqa: E402

F32_MAX = float(np.finfo(np.float32).max)
F32_TINY = float(np.finfo(np.float32).tiny)           # smallest normal
F32_DENORM_MIN = 2.0 ** -149


def same_bits(out32, out64, what=""):
    """out32 (float32) == float32(out64), NaN positions equal, everything else compared as int32."""
    a = out64.cpu().numpy() if isinstance(out64, torch.Tensor) else np.asarray(out64)
    b = out32.cpu().numpy() if isinstance(out32, torch.Tensor) else np.asarray(out32)
    assert a.dtype == np.float64 and b.dtype == np.float32, (what, a.dtype, b.dtype)
    assert a.shape == b.shape, what
    with np.errstate(over="ignore", under="ignore"):
        want = a.astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(b)), what
    assert np.array_equal(want.view(np.int32)[~nan], b.view(np.int32)[~nan]), what


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


@pytest.fixture()
def heng():
    from camera_linearity_amd.measurand import _HOST_ENGINE
    return _HOST_ENGINE


def both(heng, frames, t, icrf, diff, stds=None, **kw):
    """The same host merge with float64 and with float32 outputs; checks the pair and returns (out64, out32)."""
    fr = [T(f) for f in frames]
    sd = None if stds is None else [T(s) for s in stds]
    kw = {k: (T(v) if isinstance(v, np.ndarray) and k in ("flat", "flat_std") else v) for k, v in kw.items()}
    o64 = heng.merge(fr, t, icrf, diff if sd is not None else None, sd, **kw)
    o32 = heng.merge(fr, t, icrf, diff if sd is not None else None, sd, out_dtype=torch.float32, **kw)
    assert o64.keys() == o32.keys()
    for k in o64:
        if k == "sum_w":
            assert o32[k].dtype == torch.float64 and torch.equal(o32[k], o64[k])
        else:
            same_bits(o32[k], o64[k], k)
    return o64, o32


# ---------------------------------------------------------------------------------------------- dispatch (HIP library, dry)
def _describe(n=7, C_=3, H=64, W=64, std=False, flat=False, sumw=False, f64=False, variant=0, align=0, darks=False, hot_ws=False,
              frames_ws=False, struct_size=None, out_kind=1, out_align=0):
    """The helper of tests/test_host_logic.py::test_merge_dispatch_table with out_kind (and an offset of the output pointers)."""
    from camera_linearity_amd import _native as nat
    a = nat.MergeArgs()
    a.struct_size = C.sizeof(nat.MergeArgs) if struct_size is None else struct_size
    a.n_frames, a.channels, a.variant = n, C_, variant
    a.out_kind = out_kind
    a.height = a.rows = a.buf_rows = H
    a.width = W
    base = 1 << 20
    fr = (C.c_void_p * n)(*[base * (i + 1) + align for i in range(n)])
    if f64:
        a.frames_f64 = C.cast(fr, C.POINTER(C.c_void_p))
    else:
        a.frames_u8 = C.cast(fr, C.POINTER(C.c_void_p))
    ex = (C.c_double * n)(*[1e-3 * 2 ** i for i in range(n)])
    a.exposures = C.cast(ex, C.POINTER(C.c_double))
    a.icrf, a.w_lut, a.out_val = base * 40, base * 41, base * 42 + out_align
    keep = [fr, ex]
    if std:
        sd = (C.c_void_p * n)(*[base * (50 + i) for i in range(n)])
        a.stds = C.cast(sd, C.POINTER(C.c_void_p))
        a.icrf_diff, a.dw_lut, a.out_std = base * 43, base * 44, base * 45 + out_align
        keep.append(sd)
    if flat:
        a.flat_u8 = base * 46
        a.flat_std = base * 47
    if sumw:
        a.out_sum_w = base * 48
    if darks:
        dk = (C.c_void_p * n)(*[base * 90 for _ in range(n)])
        dm = (C.c_int32 * n)(*[13] * n)
        a.darks_u8 = C.cast(dk, C.POINTER(C.c_void_p))
        a.dark_min_dn = C.cast(dm, C.POINTER(C.c_int32))
        a.median_k = 3
        keep += [dk, dm]
        if hot_ws:
            a.hot_workspace, a.hot_workspace_bytes = base * 91, nat.lib.hm_merge_hot_workspace_bytes(H * W * C_)
    if frames_ws:
        a.frames_workspace, a.frames_workspace_bytes = base * 92, 8 * H * W * C_
    buf = C.create_string_buffer(1024)
    rc = nat.lib.hm_merge_describe(C.byref(a), buf, 1024)
    return rc, buf.value.decode(), int(nat.lib.hm_merge_algorithmic_bytes(C.byref(a)))


# the one-launch argument sets of test_merge_dispatch_table, with the kernel family a float32 call must name
SINGLE_LAUNCH = [
    (dict(n=7), ["merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32x4>"]),                       # four float32 per lane: 16-byte stores
    (dict(n=8), ["merge_u8_loop<C=3,flat=0,sum_w=0,out=f32>(N=8)"]),                    # float32: N = 7 and 15 are templated, the others stream at run-time N
    (dict(n=15), ["merge_u8_val3<N=15,U=3,PF=0,MAP=0,out=f32>"]),
    (dict(n=7, H=4, W=8), ["merge_generic<f64in=0,std=0,out=f32>"]),
    (dict(n=7, H=5, W=64), ["merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32x4>", "merge_generic<f64in=0,std=0,out=f32>"]),
    (dict(n=7, variant=32), ["merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32>"]),              # the A/B switch: the same kernel with pair stores
    (dict(n=7, align=2), ["merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32>"]),                 # frames 2- but not 4-byte aligned: no dword loads
    (dict(n=7, std=True), ["merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,out=f32>"]),
    (dict(n=7, std=True, flat=True, darks=True), ["merge_u8_fast_std<N=7,U=1,flat=1,sum_w=0,out=f32>", "merge_fixup_hot<f64in=0,std=1,out=f32>"]),
    (dict(n=7, std=True, darks=True, hot_ws=True), ["merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,out=f32>", "merge_scan_hot", "merge_patch_hot<f64in=0,std=1,out=f32>"]),
    (dict(n=7, sumw=True), ["merge_u8_fast<N=7,U=2,flat=0,sum_w=1,out=f32>"]),
    (dict(n=7, flat=True), ["merge_u8_val3<N=7,U=2,PF=1,MAP=3,flat=1,out=f32x4>"]),
    (dict(n=15, flat=True), ["merge_u8_val3<N=15,U=2,PF=1,MAP=0,flat=1,out=f32x4>"]),
    (dict(n=7, flat=True, sumw=True), ["merge_u8_fast<N=7,U=2,flat=1,sum_w=1,out=f32>"]),
    (dict(n=17), ["merge_u8_loop<C=3,flat=0,sum_w=0,out=f32>(N=17)"]),
    (dict(n=20, std=True), ["merge_u8_loop_std<C=3,flat=0,sum_w=0,out=f32>(N=20)"]),
    (dict(n=21), ["merge_u8_loop<C=3,flat=0,sum_w=0,out=f32>(N=21)"]),
    (dict(n=32, std=True), ["merge_u8_loop_std<C=3,flat=0,sum_w=0,out=f32>(N=32)"]),
    (dict(n=7, C_=1), ["merge_u8_val3<N=7,U=4,PF=1,MAP=3,C=1,out=f32x4>"]),
    (dict(n=7, C_=1, flat=True), ["merge_u8_val3<N=7,U=2,PF=1,MAP=3,flat=1,C=1,out=f32x4>"]),
    (dict(n=7, C_=1, std=True), ["merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,C=1,out=f32>"]),
    (dict(n=7, C_=1, std=True, flat=True), ["merge_u8_fast_std<N=7,U=1,flat=1,sum_w=0,C=1,out=f32>"]),
    (dict(n=7, C_=1, std=True, sumw=True), ["merge_u8_loop_std<C=1,flat=0,sum_w=1,out=f32>(N=7)"]),
    (dict(n=17, C_=1), ["merge_u8_loop<C=1,flat=0,sum_w=0,out=f32>(N=17)"]),
    (dict(n=7, C_=2), ["merge_u8_loop<C=2,flat=0,sum_w=0,out=f32>(N=7)"]),
    (dict(n=7, f64=True, std=True), ["merge_f64_std<C=3,flat=0,sum_w=0,out=f32>(N=7)"]),
    (dict(n=7, f64=True), ["merge_f64_val<C=3,flat=0,sum_w=0,out=f32>(N=7)"]),
    (dict(n=7, align=1), ["merge_generic<f64in=0,std=0,out=f32>"]),
    (dict(n=7, variant=-1), ["merge_generic<f64in=0,std=0,out=f32>"]),
    (dict(n=7, variant=1120), ["merge_u8_fast<N=7,U=2,flat=0,sum_w=0,out=f32>"]),
]


@pytest.mark.parametrize("kw,want", SINGLE_LAUNCH, ids=[str(i) for i in range(len(SINGLE_LAUNCH))])
def test_f32_dispatch_names_every_storing_kernel(kw, want):
    from camera_linearity_amd import _native as nat
    rc, names, bytes32 = _describe(**kw)
    assert rc == nat.HM_OK, (kw, rc)
    assert names.split(" + ") == want
    for part in names.split(" + "):                        # every kernel that stores val / std says out=f32 (the dark-map scan stores neither)
        assert "out=f32" in part or part == "merge_scan_hot", names
    # the float64 twin of the same call: its string has no trace of the new field, and it moves 4 more bytes per val / std element
    rc64, names64, bytes64 = _describe(out_kind=0, **dict(kw, variant=0 if kw.get("variant") == 32 else kw.get("variant", 0)))
    assert rc64 == nat.HM_OK and "out=" not in names64
    E = kw.get("H", 64) * kw.get("W", 64) * kw.get("C_", 3)
    assert bytes64 - bytes32 == 4 * E * (2 if kw.get("std") else 1)


def test_f32_dispatch_refusals():
    from camera_linearity_amd import _native as nat
    assert _describe(7, out_kind=2)[0] == nat.HM_EINVAL and _describe(7, out_kind=-1)[0] == nat.HM_EINVAL
    assert _describe(33, frames_ws=True)[0] == nat.HM_EUNSUPPORTED                          # the chunked path keeps float64 running sums in out_val
    assert _describe(33, frames_ws=True, out_kind=0)[0] == nat.HM_OK
    assert _describe(7, variant=-3, frames_ws=True)[0] == nat.HM_EUNSUPPORTED
    assert _describe(7, H=65538, W=21846)[0] == nat.HM_EUNSUPPORTED                         # 2^32 elements or more: the row-band loop is float64 only
    assert _describe(7, H=65538, W=21846, out_kind=0)[0] == nat.HM_OK
    # the two ABI-1 layouts have no out_kind: whatever lies in that word, they mean float64
    for size in (264, 280):
        assert _describe(7, struct_size=size, out_kind=1)[:2] == (0, "merge_u8_val3<N=7,U=4,PF=1,MAP=3>")
        assert _describe(7, struct_size=size, out_kind=77)[:2] == (0, "merge_u8_val3<N=7,U=4,PF=1,MAP=3>")
        assert _describe(7, struct_size=size, out_kind=1)[2] == _describe(7, out_kind=0)[2]
    # alignment: float32 outputs need 4 bytes; 8 bytes at the first element for the streaming kernels, else the generic kernel
    assert _describe(7, out_align=2)[0] == nat.HM_EALIGN
    assert _describe(7, std=True, out_align=2)[0] == nat.HM_EALIGN
    assert _describe(7, out_align=4)[:2] == (0, "merge_generic<f64in=0,std=0,out=f32>")
    assert _describe(7, out_align=8)[:2] == (0, "merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32>")     # pairs; four per lane need 16 bytes
    assert _describe(7, out_align=16)[:2] == (0, "merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32x4>")
    assert _describe(7, variant=32, out_kind=0)[0] == nat.HM_EINVAL                               # the switch exists for float32 calls only
    assert _describe(7, out_align=8, out_kind=0)[:2] == (0, "merge_generic<f64in=0,std=0>")  # float64 pairs are 16 bytes
    assert _describe(7, out_align=4, out_kind=0)[0] == nat.HM_EALIGN


def test_f32_algorithmic_bytes_host_and_device_builds_agree():
    from camera_linearity_amd import _native as nat
    a = nat.MergeArgs()
    a.struct_size = C.sizeof(nat.MergeArgs)
    a.n_frames, a.channels, a.height, a.width, a.rows, a.buf_rows = 7, 3, 10, 12, 10, 12
    one = (C.c_void_p * 7)(*[4096] * 7)
    a.frames_u8 = C.cast(one, C.POINTER(C.c_void_p))
    a.out_val = 8192
    for lib in (nat.hip_lib, nat.host_lib()):
        a.out_kind, a.stds, a.out_std = 0, None, None
        assert lib.hm_merge_algorithmic_bytes(C.byref(a)) == 360 * (7 + 8)
        a.out_kind = 1
        assert lib.hm_merge_algorithmic_bytes(C.byref(a)) == 360 * (7 + 4)                # config 2's 11 bytes per element
        a.stds, a.out_std = C.cast(one, C.POINTER(C.c_void_p)), 16384
        assert lib.hm_merge_algorithmic_bytes(C.byref(a)) == 360 * (7 * 9 + 8)            # the std form: 71
        a.out_kind = 0
        assert lib.hm_merge_algorithmic_bytes(C.byref(a)) == 360 * (7 * 9 + 16)           # 79


# ---------------------------------------------------------------------------------------------- equality on the host build
@pytest.mark.parametrize("shape", [(4, 8), (5, 64), (11, 5), (40, 52)])
@pytest.mark.parametrize("n", [1, 2, 7, 21, 32])
def test_host_f32_equals_cast_u8_and_f64_frames(heng, shape, n):
    h, w = shape
    frames, stds, t = orc.synthetic_stack(400 + n, n, h, w, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    both(heng, frames, t, icrf, diff)
    both(heng, frames, t, icrf, diff, stds, want_sum_w=True)
    f64 = [orc.unit_from_u8(f) + 1e-4 * (i + 1) for i, f in enumerate(frames)]
    both(heng, f64, t, icrf, diff)
    both(heng, f64, t, icrf, diff, stds)


@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
@pytest.mark.parametrize("flat_u8", [True, False])
def test_host_f32_equals_cast_channels_flat_and_sum_of_weights(heng, Cc, flat_u8):
    n, h, w = 7, 40, 52
    frames, stds, t = orc.synthetic_stack(420 + Cc, n, h, w, c=Cc, with_std=True)
    icrf = np.stack([np.linspace(0, 1, 256) ** (1.5 + 0.2 * k) for k in range(Cc)], axis=1)
    diff = orc.icrf_derivative(icrf)
    rng = np.random.default_rng(Cc)
    flat = rng.integers(180, 230, size=(h, w, Cc)).astype(np.uint8)
    if not flat_u8:
        flat = orc.unit_from_u8(flat) + 1e-3
    kw = dict(flat=flat, ff_mean=[0.8, 0.81, 0.79, 0.82][:Cc])
    both(heng, frames, t, icrf, diff, **kw)
    both(heng, frames, t, icrf, diff, want_sum_w=True, **kw)
    both(heng, frames, t, icrf, diff, stds, flat_std=np.full((h, w, Cc), 0.002), ff_std_mean=[0.002] * Cc, want_sum_w=True, **kw)
    o64, o32 = both(heng, frames, t, icrf, diff, want_sum_w=True, want_val=False)          # sum of weights alone: nothing is float32
    assert list(o32) == ["sum_w"]


@pytest.mark.parametrize("hot_queue", [True, False])
def test_host_f32_equals_cast_dark_maps(heng, hot_queue):
    n, h, w = 7, 40, 52
    frames, stds, t = orc.synthetic_stack(431, n, h, w, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    rng = np.random.default_rng(5)
    d = rng.integers(0, 10, size=(h, w, 3)).astype(np.uint8)
    d[rng.random(d.shape) < 0.03] = 200
    d[0, 0, 0] = d[h - 1, w - 1, 2] = d[0, w - 1, 1] = 255
    darks = [None] + [T(d)] * (n - 1)
    mins = [256] + [100] * (n - 1)
    both(heng, frames, t, icrf, diff, stds, darks=darks, dark_min=mins, median_k=3, hot_queue=hot_queue)
    both(heng, frames, t, icrf, diff, darks=darks, dark_min=mins, median_k=5, hot_queue=hot_queue)


def test_host_f32_row_tiles_empty_tile_and_one_pixel(heng):
    n, h, w = 3, 11, 5
    frames, stds, t = orc.synthetic_stack(440, n, h, w, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    _, whole = both(heng, frames, t, icrf, diff, stds)
    for r0, r1 in ((1, 4), (3, 11), (0, 1), (10, 11)):                                      # odd row offsets: W * C = 15 elements per row
        _, part = both(heng, frames, t, icrf, diff, stds, height=h, row0=r0, rows=r1 - r0)
        for k in ("val", "std"):
            assert torch.equal(part[k], whole[k][r0:r1]), (r0, r1, k)
    out = heng.merge([T(f) for f in frames], t, icrf, diff, [T(s) for s in stds], height=h, row0=4, rows=0, out_dtype=torch.float32)
    assert out["val"].shape == (0, w, 3) and out["val"].dtype == torch.float32
    f1, s1, t1 = orc.synthetic_stack(441, 2, 1, 1, with_std=True)
    both(heng, f1, t1, icrf, diff, s1, want_sum_w=True)


def test_host_f32_range_subnormals_and_overflow(heng):
    """Results in float32's subnormal range must come out as subnormals (not flushed to zero), results beyond its maximum as +inf."""
    n, h, w = 7, 40, 52
    frames, stds, t = orc.synthetic_stack(450, n, h, w, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    # ICRF x 1e-42 with exposures >= 1e-3 s: every value below float32's smallest normal, and (where not exactly 0) above its smallest subnormal
    assert min(t) >= 1e-3
    o64, o32 = both(heng, frames, t, icrf * 1e-42, diff * 1e-42)
    v64, v32 = o64["val"].numpy(), o32["val"].numpy()
    assert v64.max() < F32_TINY and (v64 > F32_DENORM_MIN).mean() > 0.9                    # the float64 results really are in that range
    sub = v64 > F32_DENORM_MIN
    assert (v32[sub] > 0).all() and (v32[sub] < F32_TINY).all()                            # subnormals, not zeros
    both(heng, frames, t, icrf * 1e-42, diff * 1e-42, stds)                                # (the std of such a table underflows: equality only)
    # exposures x 1e-42: beyond float32's maximum
    o64, o32 = both(heng, frames, [ti * 1e-42 for ti in t], icrf, diff, stds)
    v64, v32 = o64["val"].numpy(), o32["val"].numpy()
    big = v64 > F32_MAX
    assert big.mean() > 0.9 and np.isfinite(v64).all()                                     # finite in float64, too large for float32
    assert (v32[big] == np.inf).all()


# ---------------------------------------------------------------------------------------------- Python API
def _features(t):
    return {"illumination": "bf", "magnification": "5x", "exposure": float(t), "subject": "s"}


def test_plan_outputs_dtypes_and_type_errors(heng):
    frames, stds, t = orc.synthetic_stack(460, 3, 6, 8, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    fr, sd = [T(f) for f in frames], [T(s) for s in stds]
    plan = heng.plan_merge(fr, t, icrf, diff, sd, want_sum_w=True, out_dtype=torch.float32)
    assert {k: v.dtype for k, v in plan.outputs.items()} == {"val": torch.float32, "std": torch.float32, "sum_w": torch.float64}
    assert "out=f32" in plan.kernels
    plan64 = heng.plan_merge(fr, t, icrf, diff, sd, want_sum_w=True)
    assert {v.dtype for v in plan64.outputs.values()} == {torch.float64} and "out=" not in plan64.kernels
    assert plan64.algorithmic_bytes - plan.algorithmic_bytes == 4 * 6 * 8 * 3 * 2
    for bad in (torch.float16, torch.bfloat16, torch.int32, None, "float32"):
        with pytest.raises(TypeError):
            heng.plan_merge(fr, t, icrf, diff, sd, out_dtype=bad)
    # more than HM_MAX_FRAMES frames: refused for float32 (no silent float64), still served for float64
    f33, _, t33 = orc.synthetic_stack(461, 33, 4, 4)
    with pytest.raises(NotImplementedError):
        heng.merge([T(f) for f in f33], t33, icrf, out_dtype=torch.float32)
    assert heng.merge([T(f) for f in f33], t33, icrf)["val"].dtype == torch.float64
    from camera_linearity_amd.parallel import RowTileSet
    with pytest.raises(TypeError):
        RowTileSet(6, 1).add_tile(0, fr, t, icrf, out_dtype=torch.float32)


def test_process_hdr_image_f32_measurand_ops_and_saves(tmp_path):
    from camera_linearity_amd import tiff_io
    from camera_linearity_amd.exposure_series import ExposureSeries
    from camera_linearity_amd.image_set import ImageSet
    frames, stds, t = orc.synthetic_stack(470, 5, 24, 20, with_std=True)
    icrf, diff = orc.synthetic_icrf()

    def run(out_dtype):
        sets = [ImageSet(value=f, std=s.copy(), features=_features(ti)) for f, s, ti in zip(frames, stds, t)]
        series = ExposureSeries(input_image_sets=sets)
        series.process_HDR_image(icrf, diff, out_dtype=out_dtype)
        return series.merged_image_set
    hdr64, hdr32, hdr_none = run(torch.float64), run(torch.float32), run(None)
    m64, m32 = hdr64.measurand, hdr32.measurand
    assert m32.backend == "numpy" and m32.val.dtype == np.float32 and m32.std.dtype == np.float32
    assert hdr_none.measurand.val.dtype == np.float64 and np.array_equal(hdr_none.measurand.val, m64.val)
    same_bits(m32.val, m64.val, "val")
    same_bits(m32.std, m64.std, "std")
    # a float32 Measurand is storage: operators upcast val AND std and compute in float64
    from camera_linearity_amd.measurand_factory import Measurand
    up = Measurand(m32.val.astype(np.float64), m32.std.astype(np.float64), use_cupy=False)
    for got, want in ((m32 * 2.0, up * 2.0), (m32 - m64, up - m64), (m32 ** 2, up ** 2), (-m32, -up)):
        assert got.val.dtype == np.float64 and got.std.dtype == np.float64
        assert np.array_equal(got.val, want.val) and np.array_equal(got.std, want.std)
    st32, stup = m32.compute_dimension_statistics(axis=(0, 1)), up.compute_dimension_statistics(axis=(0, 1))
    assert all(np.array_equal(st32[k], stup[k]) for k in st32)
    # save_32bit: the float32 arrays bit for bit, under 32bit/ with save_64bit's names
    hdr32.path = tmp_path / "s bf 5x.tif"
    hdr32.save_32bit(is_HDR=True)
    back = tiff_io.imread(tmp_path / "32bit" / "s bf 5x HDR.tif", tiff_io.IMREAD_UNCHANGED)
    back_std = tiff_io.imread(tmp_path / "32bit" / "s bf 5x HDR STD.tif", tiff_io.IMREAD_UNCHANGED)
    assert back.dtype == np.float32 and np.array_equal(back.view(np.int32), m32.val.view(np.int32))
    assert back_std.dtype == np.float32 and np.array_equal(back_std.view(np.int32), m32.std.view(np.int32))
    hdr32.save_32bit(tmp_path / "sep" / "x.tif", separate_channels=True)
    from camera_linearity_amd import settings as gs
    one = tiff_io.imread(tmp_path / "sep" / f"x {gs.CH_STR.get(1, '1')}.tif", tiff_io.IMREAD_UNCHANGED)
    assert one.dtype == np.float32 and np.array_equal(one, m32.val[:, :, 1])
    hdr64.path = tmp_path / "d bf 5x.tif"
    hdr64.save_32bit()                                                                       # a float64 result is rounded on the way out
    same_bits(tiff_io.imread(tmp_path / "32bit" / "d bf 5x.tif", tiff_io.IMREAD_UNCHANGED), m64.val)
    # save_64bit of a float32 result: the upcast, whole image and per channel
    hdr32.save_64bit(tmp_path / "w" / "y.tif", is_HDR=True)
    hdr32.save_64bit(tmp_path / "w" / "z.tif", separate_channels=True)
    b64 = tiff_io.imread(tmp_path / "w" / "y HDR.tif", tiff_io.IMREAD_UNCHANGED)
    assert b64.dtype == np.float64 and np.array_equal(b64, m32.val.astype(np.float64))
    c64 = tiff_io.imread(tmp_path / "w" / f"z STD {gs.CH_STR.get(2, '2')}.tif", tiff_io.IMREAD_UNCHANGED)
    assert c64.dtype == np.float64 and np.array_equal(c64, m32.std[:, :, 2].astype(np.float64))
    hdr32.save_8bit(tmp_path / "e" / "q.tif")
    hdr64.save_8bit(tmp_path / "e" / "r.tif")
    assert tiff_io.imread(tmp_path / "e" / "q.tif", tiff_io.IMREAD_UNCHANGED).dtype == np.uint8
