"""The fused merge reading float32 std frames as they are (hm_merge_std_f32, engine.plan_merge with torch.float32 stds), CPU part: the host
build of the C ABI, the dry dispatch and the argument checks of the HIP library, and the Python surface. No GPU needed.

The criterion is exact: widening float32 to float64 loses nothing, so the float32-std merge equals the float64-std merge of the widened
frames, compared as integer bit patterns (NaN positions must coincide). Stds are random float32 with about 5 % exact zeros, one subnormal
(1e-45), one 3e38 and - in cases without dark maps, a median of NaNs has no defined answer - one +inf and one NaN."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import hdr_oracle as orc  # noqa: E402

F32 = torch.float32


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


def assert_same_bits(a, b, what=""):
    """NaN positions coincide, every other element has the same bit pattern."""
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), what
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    assert torch.equal(a.contiguous().view(it)[~na], b.contiguous().view(it)[~nb]), what


@pytest.fixture()
def heng():
    from camera_linearity_amd.measurand import _HOST_ENGINE
    return _HOST_ENGINE


def make_stds(rng, n, shape, specials=True, nonfinite=True):
    out = []
    for _ in range(n):
        s = rng.random(shape, dtype=np.float32) * np.float32(0.02)
        s[rng.random(shape) < 0.05] = 0.0
        out.append(s)
    if specials and out[0].size >= 4:
        flat = out[0].reshape(-1)
        flat[1] = np.float32(1e-45)                        # the smallest float32 subnormal
        out[-1].reshape(-1)[2] = np.float32(3e38)
        if nonfinite:
            flat[3] = np.inf
            out[n // 2].reshape(-1)[0] = np.nan
    return out


def make_icrf(c):
    icrf = np.stack([np.linspace(0, 1, 256) ** (1.6 + 0.2 * k) for k in range(c)], axis=1)
    return icrf, orc.icrf_derivative(icrf)


def make_frames(rng, n, h, w, c, f64=False):
    dn = [rng.integers(0, 256, size=(h, w, c)).astype(np.uint8) for _ in range(n)]
    if not f64:
        return dn
    out = []
    for f in dn:
        v = (f.astype(np.float64) + rng.choice([0.0, 0.5, 0.25, -0.25], size=f.shape)) / 255.0
        v[rng.random(f.shape) < 0.05] += 1.0
        out.append(v)
    return out


def f32_vs_f64(heng, frames, t, icrf, diff, sd32, **kw):
    """Host build: the float32-std plan (hm_merge_std_f32) against the plan fed the widened stds (hm_merge). -> the float32-std plan's outputs."""
    from camera_linearity_amd import _native as nat
    fr = [T(f) for f in frames]
    s32 = [T(s) for s in sd32]
    assert all(s.dtype == F32 for s in s32)
    kw = {k: (T(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    if "darks" in kw:
        kw["darks"] = [T(d) for d in kw["darks"]]
    p64 = heng.plan_merge(fr, t, icrf, diff, [s.to(torch.float64) for s in s32], **kw)
    p32 = heng.plan_merge(fr, t, icrf, diff, s32, **kw)
    assert "std=f32" in p32.kernels and "std=f32" not in p64.kernels
    assert not p32.args.stds and p64.args.stds                                     # the float32 frames travel beside the struct
    assert all(k.data_ptr() == s.data_ptr() for k, s in zip([x for x in p32._keep if isinstance(x, torch.Tensor) and x.dtype == F32], s32))   # taken as they are
    lib = nat.host_lib()
    calls = lib.calls["hm_merge_std_f32"]
    for v in p32.outputs.values():
        v.fill_(float("nan"))
    p64.launch()
    p32.launch()
    assert lib.calls["hm_merge_std_f32"] == calls + 1
    assert p32.outputs.keys() == p64.outputs.keys() and "std" in p32.outputs
    for k in p64.outputs:
        assert_same_bits(p32.outputs[k], p64.outputs[k], k)
    assert p64.algorithmic_bytes - p32.algorithmic_bytes == 4 * len(fr) * p32.outputs["val"].numel()
    return p32.outputs


# ---------------------------------------------------------------------------------------------- host build against its float64-std route
@pytest.mark.parametrize("n", [1, 7, 15, 20, 32])
def test_host_96x130(heng, n):
    h, w, c = 96, 130, 3
    rng = np.random.default_rng(2000 + n)
    frames = make_frames(rng, n, h, w, c)
    t = list(1e-3 * 1.2 ** np.arange(n))
    icrf, diff = make_icrf(c)
    sd = make_stds(rng, n, (h, w, c))
    flat = dict(flat=rng.integers(180, 230, size=(h, w, c)).astype(np.uint8), flat_std=np.full((h, w, c), 0.002), ff_mean=[0.8, 0.81, 0.79],
                ff_std_mean=[0.002] * c)
    out = f32_vs_f64(heng, frames, t, icrf, diff, sd)
    assert torch.isnan(out["std"]).any() and float((out["std"] > 0).double().mean()) > 0.5
    f32_vs_f64(heng, frames, t, icrf, diff, sd, want_sum_w=True, **flat)
    o32 = f32_vs_f64(heng, frames, t, icrf, diff, sd, out_dtype=F32, **flat)
    assert o32["std"].dtype == F32


@pytest.mark.parametrize("c", [1, 2, 4])
def test_host_channel_counts(heng, c):
    n, h, w = 7, 40, 52
    rng = np.random.default_rng(2100 + c)
    icrf, diff = make_icrf(c)
    f32_vs_f64(heng, make_frames(rng, n, h, w, c), list(1e-3 * 1.3 ** np.arange(n)), icrf, diff, make_stds(rng, n, (h, w, c)), want_sum_w=True)


def test_host_float64_frames(heng):
    n, h, w, c = 5, 40, 52, 3
    rng = np.random.default_rng(2200)
    icrf, diff = make_icrf(c)
    frames = make_frames(rng, n, h, w, c, f64=True)
    t = list(1e-3 * 1.3 ** np.arange(n))
    f32_vs_f64(heng, frames, t, icrf, diff, make_stds(rng, n, (h, w, c)))
    f32_vs_f64(heng, frames, t, icrf, diff, make_stds(rng, n, (h, w, c)), out_dtype=F32)


def _dark_map(rng, h, w, c, density=0.01):
    d = rng.integers(0, 10, size=(h, w, c)).astype(np.uint8)
    d[rng.random(d.shape) < density] = 200
    for y, x, ch in ((0, 0, 0), (0, w - 1, 1), (h - 1, 0, c - 1), (h - 1, w - 1, 0), (h // 2, 0, 1), (h // 2 + 1, w - 1, c - 1)):
        d[y, x, ch] = 255                                  # hot pixels on the image border: reflect
    return d


@pytest.mark.parametrize("k", [3, 7])
def test_host_dark_maps(heng, k):
    n, h, w, c = 7, 64, 64, 3
    rng = np.random.default_rng(2300 + k)
    icrf, diff = make_icrf(c)
    frames = make_frames(rng, n, h, w, c)
    d = _dark_map(rng, h, w, c)
    sd = make_stds(rng, n, (h, w, c), nonfinite=False)
    t = list(1e-3 * 1.3 ** np.arange(n))
    # the same map for every frame: every hot element is hot in two (and more) frames at once
    f32_vs_f64(heng, frames, t, icrf, diff, sd, darks=[d] * n, dark_min=[100] * n, median_k=k)
    f32_vs_f64(heng, frames, t, icrf, diff, sd, darks=[None] + [d] * (n - 1), dark_min=[256] + [100] * (n - 1), median_k=k, want_sum_w=True,
               out_dtype=F32)


def test_host_row_tiles(heng):
    """3 tiles of a 67-row image with dark maps (buf_row0 halo) equal the whole-image call."""
    n, h, w, c = 7, 67, 20, 3
    rng = np.random.default_rng(2400)
    icrf, diff = make_icrf(c)
    frames = make_frames(rng, n, h, w, c)
    d = _dark_map(rng, h, w, c, density=0.03)
    d[22, 5, 1] = d[23, 5, 1] = d[44, 7, 0] = d[45, 7, 0] = 255         # hot on both sides of the tile seams
    sd = make_stds(rng, n, (h, w, c), nonfinite=False)
    t = list(1e-3 * 1.3 ** np.arange(n))
    dk, mins = [None, None] + [d] * (n - 2), [256, 256] + [100] * (n - 2)
    whole = f32_vs_f64(heng, frames, t, icrf, diff, sd, darks=dk, dark_min=mins, median_k=3)
    for r0, r1 in ((0, 23), (23, 45), (45, 67)):
        b0, b1 = max(0, r0 - 1), min(h, r1 + 1)
        part = f32_vs_f64(heng, [f[b0:b1] for f in frames], t, icrf, diff, [s[b0:b1] for s in sd],
                          darks=[None if x is None else x[b0:b1] for x in dk], dark_min=mins, median_k=3, height=h, row0=r0, rows=r1 - r0, buf_row0=b0)
        for key in part:
            assert_same_bits(part[key], whole[key][r0:r1], (r0, key))


def test_host_random_calls(heng):
    """About 200 small random calls - shape, N, C, options, special std values - against the host build's own float64-std route."""
    rng = np.random.default_rng(2500)
    for it in range(200):
        c = int(rng.integers(1, 5))
        n = int(rng.choice([1, 2, 3, 5, 7, 8, 15, 17, 32]))
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        f64 = bool(rng.random() < 0.3)
        hot = bool(rng.random() < 0.4) and h >= 2 and w >= 2
        icrf, diff = make_icrf(c)
        frames = make_frames(rng, n, h, w, c, f64)
        sd = make_stds(rng, n, (h, w, c), specials=bool(rng.random() < 0.7), nonfinite=not hot)
        kw = {}
        if hot:
            d = (rng.random((h, w, c)) < 0.2).astype(np.uint8) * 255
            kw.update(darks=[d if rng.random() < 0.7 else None for _ in range(n)], dark_min=[100] * n, median_k=int(rng.choice([3, 5, 7])))
        if rng.random() < 0.5:
            kw.update(flat=rng.integers(150, 230, size=(h, w, c)).astype(np.uint8), flat_std=np.full((h, w, c), 0.002),
                      ff_mean=[0.8, 0.81, 0.79, 0.82][:c], ff_std_mean=[0.002] * c)
        if rng.random() < 0.5:
            kw.update(want_sum_w=True)
        if rng.random() < 0.5:
            kw.update(out_dtype=F32)
        f32_vs_f64(heng, frames, list(1e-3 * 1.3 ** np.arange(n)), icrf, diff, sd, **kw)


# ---------------------------------------------------------------------------------------------- dispatch and validation (HIP library, dry)
BASE = 1 << 20


def _args(n=7, C_=3, H=64, W=64, flat=False, sumw=False, f64=False, variant=0, darks=False, hot_ws=False, struct_size=None, out_kind=0,
          stream_std=False, row0=0, buf_rows=None):
    """Fake, aligned pointers: hm_*_describe runs the library's own dispatch with launching switched off. stream_std: args->stds set."""
    from camera_linearity_amd import _native as nat
    a = nat.MergeArgs()
    a.struct_size = C.sizeof(nat.MergeArgs) if struct_size is None else struct_size
    a.n_frames, a.channels, a.variant = n, C_, variant
    a.out_kind = out_kind
    a.height = a.buf_rows = H
    a.row0, a.rows = row0, H - row0
    a.width = W
    fr = (C.c_void_p * n)(*[BASE * (i + 1) for i in range(n)])
    if f64:
        a.frames_f64 = C.cast(fr, C.POINTER(C.c_void_p))
    else:
        a.frames_u8 = C.cast(fr, C.POINTER(C.c_void_p))
    ex = (C.c_double * n)(*[1e-3 * 1.2 ** i for i in range(n)])
    a.exposures = C.cast(ex, C.POINTER(C.c_double))
    a.icrf, a.w_lut, a.out_val = BASE * 40, BASE * 41, BASE * 42
    a.icrf_diff, a.dw_lut, a.out_std = BASE * 43, BASE * 44, BASE * 45
    keep = [fr, ex]
    if stream_std:
        sd = (C.c_void_p * n)(*[BASE * (50 + i) for i in range(n)])
        a.stds = C.cast(sd, C.POINTER(C.c_void_p))
        keep.append(sd)
    if flat:
        a.flat_u8, a.flat_std = BASE * 46, BASE * 47
    if sumw:
        a.out_sum_w = BASE * 48
    if darks:
        dk = (C.c_void_p * n)(*[BASE * 90 for _ in range(n)])
        dm = (C.c_int32 * n)(*[13] * n)
        a.darks_u8 = C.cast(dk, C.POINTER(C.c_void_p))
        a.dark_min_dn = C.cast(dm, C.POINTER(C.c_int32))
        a.median_k = 3
        keep += [dk, dm]
        if hot_ws:
            a.hot_workspace, a.hot_workspace_bytes = BASE * 91, nat.hip_lib.hm_merge_hot_workspace_bytes(H * W * C_)
    a._keep = keep
    return a


def _stds(n=7, offset=0):
    return (C.c_void_p * n)(*[BASE * (50 + i) + offset for i in range(n)])


def _describe(lib, a, sd):
    buf = C.create_string_buffer(1024)
    rc = lib.hm_merge_std_f32_describe(C.byref(a), sd, C.addressof(buf), 1024)
    return rc, buf.value.decode()


DISPATCH = [
    (dict(n=7), 0, ["merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,std=f32>"]),
    (dict(n=7, flat=True), 0, ["merge_u8_fast_std<N=7,U=1,flat=1,sum_w=0,std=f32>"]),
    (dict(n=15), 0, ["merge_u8_fast_std<N=15,U=1,flat=0,sum_w=0,std=f32>"]),
    (dict(n=15, flat=True), 0, ["merge_u8_fast_std<N=15,U=1,flat=1,sum_w=0,std=f32>"]),
    (dict(n=7, out_kind=1), 0, ["merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,std=f32,out=f32>"]),
    (dict(n=15, flat=True, out_kind=1), 0, ["merge_u8_fast_std<N=15,U=1,flat=1,sum_w=0,std=f32,out=f32>"]),
    (dict(n=7, sumw=True), 0, ["merge_u8_loop_std<C=3,flat=0,sum_w=1,std=f32>(N=7)"]),               # every other shape streams at run-time N
    (dict(n=15, flat=True, sumw=True), 0, ["merge_u8_loop_std<C=3,flat=1,sum_w=1,std=f32>(N=15)"]),
    (dict(n=1), 0, ["merge_u8_loop_std<C=3,flat=0,sum_w=0,std=f32>(N=1)"]),
    (dict(n=8), 0, ["merge_u8_loop_std<C=3,flat=0,sum_w=0,std=f32>(N=8)"]),
    (dict(n=16, flat=True), 0, ["merge_u8_loop_std<C=3,flat=1,sum_w=0,std=f32>(N=16)"]),
    (dict(n=20), 0, ["merge_u8_loop_std<C=3,flat=0,sum_w=0,std=f32>(N=20)"]),
    (dict(n=32, out_kind=1), 0, ["merge_u8_loop_std<C=3,flat=0,sum_w=0,std=f32,out=f32>(N=32)"]),
    (dict(n=7, C_=1), 0, ["merge_u8_loop_std<C=1,flat=0,sum_w=0,std=f32>(N=7)"]),
    (dict(n=7, C_=2), 0, ["merge_u8_loop_std<C=2,flat=0,sum_w=0,std=f32>(N=7)"]),
    (dict(n=7, C_=4, flat=True), 0, ["merge_u8_loop_std<C=4,flat=1,sum_w=0,std=f32>(N=7)"]),
    (dict(n=7, f64=True), 0, ["merge_generic<f64in=1,std=1,std=f32>"]),                              # float64 frames: the generic kernel only
    (dict(n=7, f64=True, out_kind=1), 0, ["merge_generic<f64in=1,std=1,std=f32,out=f32>"]),
    (dict(n=7, variant=-1), 0, ["merge_generic<f64in=0,std=1,std=f32>"]),
    (dict(n=7, H=5, W=64), 0, ["merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,std=f32>", "merge_generic<f64in=0,std=1,std=f32>"]),
    (dict(n=7, darks=True), 0, ["merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,std=f32>", "merge_fixup_hot<f64in=0,std=1,std=f32>"]),
    (dict(n=20, darks=True, hot_ws=True), 0, ["merge_u8_loop_std<C=3,flat=0,sum_w=0,std=f32>(N=20)", "merge_scan_hot", "merge_patch_hot<f64in=0,std=1,std=f32>"]),
    (dict(n=7, f64=True, darks=True, hot_ws=True, out_kind=1), 0,
     ["merge_generic<f64in=1,std=1,std=f32,out=f32>", "merge_scan_hot", "merge_patch_hot<f64in=1,std=1,std=f32,out=f32>"]),
    # the alignment fallbacks: std buffers that are 4- but not 8-byte aligned; a row tile with odd W * C and an odd halo
    (dict(n=7), 4, ["merge_generic<f64in=0,std=1,std=f32>"]),
    (dict(n=7, out_kind=1), 4, ["merge_generic<f64in=0,std=1,std=f32,out=f32>"]),
    (dict(n=20, H=9, W=5, row0=1), 0, ["merge_generic<f64in=0,std=1,std=f32>"]),
]


@pytest.mark.parametrize("kw,offset,names", DISPATCH, ids=[str(i) for i in range(len(DISPATCH))])
def test_f32_dispatch_names(kw, offset, names):
    from camera_linearity_amd import _native as nat
    n = kw.get("n", 7)
    a = _args(**kw)
    rc, got = _describe(nat.hip_lib, a, _stds(n, offset))
    assert rc == nat.HM_OK and got == " + ".join(names), got
    for part in got.split(" + "):
        assert "std=f32" in part or part == "merge_scan_hot"
    # the float64-std call of the same shape keeps its names, and the byte counts differ by half the std streams
    s = _args(stream_std=True, **kw)
    buf = C.create_string_buffer(1024)
    assert nat.hip_lib.hm_merge_describe(C.byref(s), buf, 1024) == nat.HM_OK and "f32>" not in buf.value.decode().replace("out=f32", "")
    E = (kw.get("H", 64) - kw.get("row0", 0)) * kw.get("W", 64) * kw.get("C_", 3)
    for lib in (nat.hip_lib, nat.host_lib()):
        assert lib.hm_merge_algorithmic_bytes(C.byref(s)) - lib.hm_merge_std_f32_algorithmic_bytes(C.byref(a)) == 4 * n * E


def test_abi_unchanged_and_symbols():
    from camera_linearity_amd import _native as nat
    assert C.sizeof(nat.MergeArgs) == 296 and nat.hip_lib.hm_version() == 2 and nat.host_lib().hm_version() == 2
    for name in ("hm_merge_std_f32", "hm_merge_std_f32_describe", "hm_merge_std_f32_algorithmic_bytes"):
        assert name in nat.EXPORTED_SYMBOLS
        for lib in (nat.hip_lib, nat.host_lib()):
            assert callable(getattr(lib, name))
    s = _args(stream_std=True)
    buf = C.create_string_buffer(256)
    assert nat.hip_lib.hm_merge_describe(C.byref(s), buf, 256) == 0 and buf.value.decode() == "merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0>"


@pytest.mark.parametrize("which", ["hip", "host"])
def test_f32_status_codes(which):
    """Every status of the specification, in its order of checks (an earlier rule wins over a later one broken in the same call)."""
    from camera_linearity_amd import _native as nat
    lib = nat.hip_lib if which == "hip" else nat.host_lib()
    buf = C.create_string_buffer(256)

    def rc(a, sd=None, n=7, offset=0):
        return lib.hm_merge_std_f32_describe(C.byref(a), _stds(n, offset) if sd is None else sd, C.addressof(buf), 256)
    # NULL args: before anything else is read (the std array is not a readable address)
    assert lib.hm_merge_std_f32(None, 8, None) == nat.HM_EINVAL
    assert lib.hm_merge_std_f32_describe(None, 8, C.addressof(buf), 256) == nat.HM_EINVAL
    assert lib.hm_merge_std_f32_algorithmic_bytes(None) == 0
    assert rc(_args()) == nat.HM_OK and "std=f32" in buf.value.decode()
    assert rc(_args(struct_size=100), offset=2) == nat.HM_EINVAL
    assert rc(_args(stream_std=True), offset=2) == nat.HM_EINVAL             # args->stds set (wins over the misaligned pointers)
    assert lib.hm_merge_std_f32_describe(C.byref(_args()), None, C.addressof(buf), 256) == nat.HM_EINVAL     # NULL stds_f32
    assert lib.hm_merge_std_f32(C.byref(_args()), None, None) == nat.HM_EINVAL
    sd = _stds(7, 2)
    sd[6] = None
    assert rc(_args(), sd) == nat.HM_EINVAL                                  # a NULL entry (wins over the misaligned ones before it)
    for field in ("icrf_diff", "dw_lut", "out_std"):
        a = _args()
        setattr(a, field, None)
        assert rc(a, offset=2) == nat.HM_EINVAL, field
    a = _args(f64=True)
    a.dw_lut = None                                                         # float64 frames need no weight tables
    assert rc(a) == nat.HM_OK
    assert rc(_args(), offset=2) == nat.HM_EALIGN                           # 2-byte misaligned std pointers
    assert lib.hm_merge_std_f32(C.byref(_args()), _stds(7, 2), None) == nat.HM_EALIGN
    assert rc(_args(n=33), n=33, offset=2) == nat.HM_EALIGN                 # ... before the frame limit
    assert rc(_args(), offset=4) == nat.HM_OK                               # 4-byte aligned is legal (the generic kernel)
    for sz in (264, 280):                                                   # the layouts of ABI version 1
        assert rc(_args(struct_size=sz)) == nat.HM_OK and "std=f32" in buf.value.decode()
    a = _args(sumw=True)                                                    # sum of weights only: hm_merge's call
    a.out_val = a.out_std = None
    assert rc(a) == nat.HM_OK and "f32" not in buf.value.decode()
    # both builds refuse what the chunked path would have to do, before any launch
    assert rc(_args(n=33), n=33) == nat.HM_EUNSUPPORTED
    assert lib.hm_merge_std_f32(C.byref(_args(n=33)), _stds(33), None) == nat.HM_EUNSUPPORTED
    for v in (-2, -3):
        assert rc(_args(variant=v)) == nat.HM_EUNSUPPORTED
        assert lib.hm_merge_std_f32(C.byref(_args(variant=v)), _stds(7), None) == nat.HM_EUNSUPPORTED
    a = _args()
    a.exposures = None                                                      # hm_merge's own rules still hold
    assert rc(a) == nat.HM_EINVAL


# ---------------------------------------------------------------------------------------------- Python surface
def test_plan_merge_dtype_rule(heng):
    """All-float32 stds are taken as they are; anything else is widened exactly as before, and the outputs are the same bits."""
    rng = np.random.default_rng(3)
    n, h, w, c = 3, 6, 7, 3
    frames = [T(f) for f in make_frames(rng, n, h, w, c)]
    t = [1e-3, 2e-3, 4e-3]
    icrf, diff = make_icrf(c)
    sd = [T(s) for s in make_stds(rng, n, (h, w, c))]
    want = heng.merge(frames, t, icrf, diff, [s.double() for s in sd])
    plan = heng.plan_merge(frames, t, icrf, diff, sd)
    assert "std=f32" in plan.kernels
    plan.launch()
    for k in want:
        assert_same_bits(plan.outputs[k], want[k], k)
    view = [torch.cat([s.reshape(-1)[:1], s.reshape(-1)]).reshape(-1)[1:].reshape(h, w, c) for s in sd]      # 4- but not 8-byte aligned views
    assert all(v.data_ptr() % 8 == 4 for v in view)
    p = heng.plan_merge(frames, t, icrf, diff, view)
    p.launch()
    assert "std=f32" in p.kernels and all(k.data_ptr() == v.data_ptr() for k, v in zip([x for x in p._keep if isinstance(x, torch.Tensor) and x.dtype == F32], view))
    for k in want:
        assert_same_bits(p.outputs[k], want[k], k)
    mixed = [sd[0], sd[1].double(), sd[2]]
    half = [s.clamp(max=6e4).half() for s in sd]
    for stds, ref in ((mixed, [s.double() for s in sd]), (half, [s.double() for s in half]), ([s.bfloat16() for s in sd], [s.bfloat16().double() for s in sd])):
        p = heng.plan_merge(frames, t, icrf, diff, stds)
        assert "f32" not in p.kernels and p.args.stds
        p.launch()
        w_ = heng.merge(frames, t, icrf, diff, ref)
        for k in w_:
            assert_same_bits(p.outputs[k], w_[k], k)
    # float32 with more frames than one launch takes, or a forced chunking: widened, as before
    many = heng.plan_merge(frames * 11, t * 11, icrf, diff, sd * 11)
    assert "f32" not in many.kernels and many.args.stds
    chunked = heng.plan_merge(frames, t, icrf, diff, sd, variant=-2)
    assert "f32" not in chunked.kernels and chunked.args.stds
    chunked.launch()
    for k in want:
        assert_same_bits(chunked.outputs[k], want[k], k)
    only_s = heng.plan_merge(frames, t, icrf, diff, sd, want_val=False, want_sum_w=True)                  # no std is formed: hm_merge's call
    only_s.launch()
    assert "f32" not in only_s.kernels and torch.equal(only_s.outputs["sum_w"], heng.merge(frames, t, icrf, want_sum_w=True)["sum_w"])


def _features(t):
    return {"illumination": "bf", "magnification": "5x", "exposure": float(t), "subject": "s"}


def test_process_hdr_image_float32_stds_on_the_host_backend(tmp_path):
    """save_32bit writes a stack's stds; from_dir_path(...).process_HDR_image(...) reads them back as float32 and merges them as they are."""
    from camera_linearity_amd import _native as nat
    from camera_linearity_amd import tiff_io
    from camera_linearity_amd.exposure_series import ExposureSeries
    from camera_linearity_amd.image_set import ImageSet
    n, h, w = 4, 16, 14
    frames, _, t = orc.synthetic_stack(91, n, h, w)
    icrf, diff = orc.synthetic_icrf()
    rng = np.random.default_rng(91)
    sd = make_stds(rng, n, (h, w, 3), nonfinite=False)
    lib = nat.host_lib()
    # stds set in memory
    sets = [ImageSet(value=f, std=s, features=_features(ti), use_cupy=False) for f, s, ti in zip(frames, sd, t)]
    calls = lib.calls["hm_merge_std_f32"]
    series = ExposureSeries(input_image_sets=sets)
    series.process_HDR_image(icrf, diff, dark_list=[], flat_list=[])
    got = series.merged_image_set.measurand
    assert lib.calls["hm_merge_std_f32"] == calls + 1
    wide = [ImageSet(value=f, std=s.astype(np.float64), features=_features(ti), use_cupy=False) for f, s, ti in zip(frames, sd, t)]
    ws = ExposureSeries(input_image_sets=wide)
    ws.process_HDR_image(icrf, diff, dark_list=[], flat_list=[])
    want = ws.merged_image_set.measurand
    assert lib.calls["hm_merge_std_f32"] == calls + 1
    assert np.array_equal(np.asarray(got.val).view(np.int64), np.asarray(want.val).view(np.int64))
    assert np.array_equal(np.asarray(got.std).view(np.int64), np.asarray(want.std).view(np.int64))
    # ... and through the files save_32bit writes
    for f, s, ti in zip(frames, sd, t):
        path = tmp_path / f"{ti * 1000:g}ms bf 5x sample.tif"
        ImageSet(value=f, std=s, features=_features(ti), use_cupy=False).save_32bit(save_path=path)
        assert tiff_io.imread(str(path).removesuffix(".tif") + " STD.tif", tiff_io.IMREAD_UNCHANGED).dtype == np.float32
        tiff_io.imwrite(path, f)                            # (save_32bit wrote the value image as float32 under this name: the DNs instead)
    from_disk = ExposureSeries.from_dir_path(tmp_path, use_cupy=False)[0]
    assert len(from_disk.input_image_sets) == n
    from_disk.process_HDR_image(icrf, diff, dark_list=[], flat_list=[])
    assert lib.calls["hm_merge_std_f32"] == calls + 2
    assert all(im.measurand._std.dtype == F32 for im in from_disk.input_image_sets)
    disk = from_disk.merged_image_set.measurand
    assert np.array_equal(np.asarray(disk.val).view(np.int64), np.asarray(want.val).view(np.int64))
    assert np.array_equal(np.asarray(disk.std).view(np.int64), np.asarray(want.std).view(np.int64))
