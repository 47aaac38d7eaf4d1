"""The fused merge on uint16 DN frames of 9- to 16-bit cameras (hm_merge_u16, hm_linearize_u16, engine.plan_merge(bit_depth=...)), CPU
part: the host build of the C ABI, the dry dispatch and the argument rules of both libraries, and the Python surface. No GPU needed.
tests/test_gpu_merge_u16.py runs the same checks (the functions below take the engine and the device) on the HIP kernels.

Three criteria:
  embedding   a uint8 stack with 256-row tables, re-expressed at depth b (DN16 = DN8 << (b - 8); tables NaN everywhere except row
              k << (b - 8) = row k of the 8-bit table) must give hm_merge's answer on the uint8 stack as integer bit patterns in val, std
              and sum_w: one operation sequence, and a wrong table index shows up as NaN. Outputs are pre-filled with NaN, none may remain.
  arithmetic  a NumPy restatement (oracle.gaussian_weight(DN / M), table gathers, the lines of oracle.merge) with the tolerances of
              tests/test_gpu_merge.py: val 1e-12, std 1e-9 relative, atol 0.
  masking     below 16 bits a few elements carry bits above the bit depth; they must behave as DN & M (the restatement masks; the embedding
              sets such bits on top of the embedded DNs)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import hdr_oracle as orc  # noqa: E402

VAL_RTOL, STD_RTOL = 1e-12, 1e-9          # tests/test_gpu_merge.py
F32, F64, U16 = torch.float32, torch.float64, torch.uint16
SHAPES = [(13, 37, 3), (8, 64, 4), (3, 43, 1), (7, 33, 2)]       # groups + tail; whole groups only; mono; two channels
DEPTHS = [9, 10, 12, 16]


def T(x, dev=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t if dev is None else t.to(dev)


def bits_of(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def assert_same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    assert not torch.isnan(got).any(), f"{what}: NaN left in the output"
    assert np.array_equal(bits_of(got), bits_of(want)), what


@pytest.fixture()
def heng():
    from camera_linearity_amd.measurand import _HOST_ENGINE
    return _HOST_ENGINE


def exposures(n):
    return list(1e-3 * 1.3 ** np.arange(n))


def gammas(c):
    return tuple(1.6 + 0.2 * k for k in range(c))


def tables8(c):
    return orc.synthetic_icrf(gammas(c))


def tables_bits(c, b):
    icrf = orc.synthetic_icrf(gammas(c), bits=2 ** b)[0]
    return icrf, orc.icrf_derivative(icrf, 2 ** b)


def make_stds(rng, n, shape):
    return [0.004 * (1 + rng.random(shape)) for _ in range(n)]          # oracle.synthetic_stack's stds


def full_range_frames(rng, n, shape, b):
    """Uniform over 0..M, element 0 = DN 0, element 1 = M; below 16 bits a few elements with bits above the depth set."""
    M = 2 ** b - 1
    out = []
    for _ in range(n):
        f = rng.integers(0, M + 1, size=shape).astype(np.uint16)
        f.reshape(-1)[0], f.reshape(-1)[1] = 0, M
        if b < 16:
            at = rng.choice(f.size, size=min(5, f.size), replace=False)
            f.reshape(-1)[at] |= np.uint16((0xFFFF << b) & 0xFFFF)
        out.append(f)
    return out


def embed_table(tab8, b):
    out = np.full((2 ** b,) + tab8.shape[1:], np.nan)
    out[np.arange(256) << (b - 8)] = tab8
    return out


def flat_kw(rng, rows, w, c, with_std):
    kw = dict(flat=0.8 + 0.05 * rng.random((rows, w, c)), ff_mean=[0.8, 0.81, 0.79, 0.82][:c])
    if with_std:
        kw.update(flat_std=np.full((rows, w, c), 0.002), ff_std_mean=[0.002] * c)
    return kw


def swap_weight_tables(plan, w, dw):
    """The plan's Gaussian weight tables (engine.weight_luts) replaced by the caller's, as a C caller passes its own."""
    plan._keep += [w, dw]
    plan.args.w_lut, plan.args.dw_lut = w.data_ptr(), dw.data_ptr()


def check_embedding(eng, dev, shape, n, b, with_std, variants=(0,), tile=None, expect=None, seed=0, **kw):
    """-> {variant: plan.kernels}. tile = (height, row0, rows, buf_row0): the frames cover rows [buf_row0, height)."""
    from camera_linearity_amd import engine
    h, w, c = shape
    rng = np.random.default_rng(1000 * b + 10 * n + c + seed)
    f8 = [rng.integers(0, 256, size=shape).astype(np.uint8) for _ in range(n)]
    for f in f8:
        f.reshape(-1)[0], f.reshape(-1)[1] = 0, 255
    f16 = [f.astype(np.uint16) << (b - 8) for f in f8]
    if b < 16:
        for f in f16:
            f.reshape(-1)[rng.choice(f.size, size=min(5, f.size), replace=False)] |= np.uint16((0xFFFF << b) & 0xFFFF)
    icrf8, diff8 = tables8(c)
    sd = [T(s, dev) for s in make_stds(rng, n, shape)] if with_std else None
    t = exposures(n)
    geo = {}
    rows = h
    if tile is not None:
        height, row0, rows, buf_row0 = tile
        assert h == height - buf_row0
        geo = dict(height=height, row0=row0, rows=rows, buf_row0=buf_row0)
    kw = {k: (T(v, dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    ref = eng.plan_merge([T(f, dev) for f in f8], t, icrf8, diff8 if with_std else None, sd, **geo, **kw)
    ref.launch()
    w8, dw8 = engine.weight_luts_host()
    ew, edw = T(embed_table(w8, b), dev), T(embed_table(dw8, b), dev)
    names = {}
    for v in variants:
        plan = eng.plan_merge([T(f, dev) for f in f16], t, embed_table(icrf8, b), embed_table(diff8, b) if with_std else None, sd,
                              bit_depth=b, variant=v, **geo, **kw)
        swap_weight_tables(plan, ew, edw)
        for o in plan.outputs.values():
            o.fill_(float("nan"))
        plan.launch()
        assert plan.outputs.keys() == ref.outputs.keys()
        for k in ref.outputs:
            assert_same_bits(plan.outputs[k], ref.outputs[k], f"{k} b={b} variant={v} {plan.kernels}")
        names[v] = plan.kernels
        if expect is not None:
            expect(v, names[v], rows * w * c)
    return names


def numpy_merge_u16(frames, b, t, icrf, diff=None, stds=None, flat=None, flat_std=None, ff_mean=None, ff_std_mean=None):
    """oracle.merge's lines on DN / M with the tables gathered at DN & M."""
    M = 2 ** b - 1
    ch = np.arange(frames[0].shape[-1])
    idx = [f.astype(np.int64) & M for f in frames]
    vals = [i.astype(np.float64) / M for i in idx]
    S = np.zeros_like(vals[0])
    for v in vals:
        S = S + orc.gaussian_weight(v)[0]
    S2 = S ** 2
    val = np.zeros_like(vals[0])
    std = None if stds is None else np.zeros_like(vals[0])
    for i, v in enumerate(vals):
        w, dw = orc.gaussian_weight(v)
        g = icrf[idx[i], ch]
        val += (w * g) / (S * t[i])
        if std is not None:
            dg = diff[idx[i], ch] * stds[i]
            std += (((dw * g + w * dg) / S - (dw * w * g) / S2) * dg / t[i]) ** 2
    if std is not None:
        std = std ** (1 / 2)
    out = dict(val=val, std=std, sum_w=S)
    if flat is not None and std is None:
        out["val"] = (val / flat) * np.asarray(ff_mean)                     # measurand.py:602
    elif flat is not None:
        out["val"], out["std"] = orc.normalize_by_map(val, std, flat, flat_std, np.asarray(ff_mean), np.asarray(ff_std_mean))
    return out


def check_arithmetic(eng, dev, shape, n, b, with_std, variant=0, with_flat=False, seed=0):
    h, w, c = shape
    rng = np.random.default_rng(7000 + 100 * b + n + c + seed)
    frames = full_range_frames(rng, n, shape, b)
    icrf, diff = tables_bits(c, b)
    sd = make_stds(rng, n, shape) if with_std else None
    t = exposures(n)
    kw = flat_kw(rng, h, w, c, with_std) if with_flat else {}
    want = numpy_merge_u16(frames, b, t, icrf, diff, sd, **kw)
    got = eng.merge([T(f, dev) for f in frames], t, icrf, diff if with_std else None, None if sd is None else [T(s, dev) for s in sd],
                    bit_depth=b, variant=variant, want_sum_w=True, **{k: (T(v, dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    np.testing.assert_allclose(got["val"].cpu().numpy(), want["val"], rtol=VAL_RTOL, atol=0)
    np.testing.assert_allclose(got["sum_w"].cpu().numpy(), want["sum_w"], rtol=VAL_RTOL, atol=0)
    if with_std:
        np.testing.assert_allclose(got["std"].cpu().numpy(), want["std"], rtol=STD_RTOL, atol=0)
    return got


def check_linearize(eng, dev, b, embedded):
    """Multi-channel and 1-D table mode: val = the gather, std = icrf_diff[idx, c] * std, idx = DN & M, all bit for bit."""
    rng = np.random.default_rng(50 + b)
    shape, M = (11, 29, 3), 2 ** b - 1
    if embedded:
        dn8 = rng.integers(0, 256, size=shape).astype(np.uint8)
        dn = dn8.astype(np.uint16) << (b - 8)
        icrf8, diff8 = tables8(3)
        icrf, diff = embed_table(icrf8, b), embed_table(diff8, b)
    else:
        dn = full_range_frames(rng, 1, shape, b)[0]
        icrf, diff = tables_bits(3, b)
    if b < 16:
        dn.reshape(-1)[::37] |= np.uint16((0xFFFF << b) & 0xFFFF)
    sd = 0.004 * (1 + rng.random(shape))
    idx = dn.astype(np.int64) & M
    ch = np.arange(3)
    for tab, dtab, gather in ((icrf, diff, lambda x: x[idx, ch]), (icrf[:, 1].copy(), diff[:, 1].copy(), lambda x: x[idx])):
        val, std, gi = eng.linearize(T(dn, dev), T(sd, dev), tab, dtab, return_index=True, bit_depth=b)
        assert gi.dtype == U16 and np.array_equal(gi.cpu().numpy().astype(np.int64), idx)
        assert np.array_equal(bits_of(val), gather(tab).view(np.int64)) and not torch.isnan(val).any()
        assert np.array_equal(bits_of(std), (gather(dtab) * sd).view(np.int64))
        v2, s2 = eng.linearize(T(dn, dev), None, tab, bit_depth=b)
        assert s2 is None and np.array_equal(bits_of(v2), bits_of(val))
        if embedded:                                        # the 8-bit call on the uint8 DNs
            tab8, dtab8 = (icrf8, diff8) if tab.ndim == 2 else (icrf8[:, 1].copy(), diff8[:, 1].copy())
            r_val, r_std = eng.linearize(T(dn8, dev), T(sd, dev), tab8, dtab8)
            assert_same_bits(val, r_val, "linearize val")
            assert_same_bits(std, r_std, "linearize std")


# ---------------------------------------------------------------------------------------------- host build
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("b", DEPTHS)
def test_host_embedding(heng, shape, b):
    rng = np.random.default_rng(b)
    h, w, c = shape
    for n, with_std in ((7, False), (9, True)):
        names = check_embedding(heng, None, shape, n, b, with_std)
        assert names[0].startswith("merge_u16_host<") and f"bits={b}" in names[0]
        check_embedding(heng, None, shape, n, b, with_std, want_sum_w=True, **flat_kw(rng, h, w, c, with_std))
        names = check_embedding(heng, None, shape, n, b, with_std, out_dtype=F32)
        assert "out=f32" in names[0]


@pytest.mark.parametrize("n", [1, 2, 32])
def test_host_embedding_frame_counts(heng, n):
    check_embedding(heng, None, (13, 37, 3), n, 12, True, want_sum_w=True)
    check_embedding(heng, None, (13, 37, 3), n, 10, False, want_val=False, want_sum_w=True)      # the sum-of-weights-only call


@pytest.mark.parametrize("tile,wc", [((16, 5, 6, 3), (37, 3)), ((16, 4, 6, 3), (37, 3))], ids=["even-offset", "odd-offset"])
def test_host_embedding_row_tiles(heng, tile, wc):
    w, c = wc
    rng = np.random.default_rng(5)
    for with_std in (False, True):
        check_embedding(heng, None, (tile[0] - tile[3], w, c), 7, 12, with_std, tile=tile, **flat_kw(rng, tile[2], w, c, with_std))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("b", DEPTHS)
def test_host_arithmetic(heng, shape, b):
    check_arithmetic(heng, None, shape, 7, b, with_std=True)
    check_arithmetic(heng, None, shape, 9, b, with_std=False, with_flat=True)
    check_arithmetic(heng, None, shape, 2, b, with_std=True, with_flat=True)


def test_host_float32_outputs_are_the_cast_float64_outputs(heng):
    """tests/test_gpu_merge_f32.py's rule."""
    rng = np.random.default_rng(11)
    shape, n, b = (13, 37, 3), 7, 12
    frames = [T(f) for f in full_range_frames(rng, n, shape, b)]
    icrf, diff = tables_bits(3, b)
    sd = [T(s) for s in make_stds(rng, n, shape)]
    o64 = heng.merge(frames, exposures(n), icrf, diff, sd, bit_depth=b)
    o32 = heng.merge(frames, exposures(n), icrf, diff, sd, bit_depth=b, out_dtype=F32)
    for k in ("val", "std"):
        assert o32[k].dtype == F32 and np.array_equal(o32[k].numpy(), o64[k].numpy().astype(np.float32))


@pytest.mark.parametrize("b", DEPTHS)
def test_host_linearize(heng, b):
    check_linearize(heng, None, b, embedded=True)
    check_linearize(heng, None, b, embedded=False)


def test_weight_tables():
    """The 16-bit grid holds the 8-bit one (k * 257 / 65535 == k / 255): the same bits there, in NumPy and in both libraries' libm tables."""
    from camera_linearity_amd import _native as nat, engine
    w8, dw8 = engine.weight_luts_host()
    assert np.array_equal(w8.view(np.int64), engine.weight_luts_host(8)[0].view(np.int64))
    w16, dw16 = engine.weight_luts_host(16)
    k = np.arange(256)
    assert np.array_equal(w16[k * 257].view(np.int64), w8.view(np.int64)) and np.array_equal(dw16[k * 257].view(np.int64), dw8.view(np.int64))
    for b in (9, 10, 12, 16):
        w, dw = engine.weight_luts_host(b)
        ow, odw = orc.gaussian_weight_lut(2 ** b)
        assert w.shape == (2 ** b,) and np.array_equal(w.view(np.int64), ow.view(np.int64)) and np.array_equal(dw.view(np.int64), odw.view(np.int64))
    tw, tdw = engine.weight_luts("cpu", 12)
    assert tw.shape == (4096,) and engine.weight_luts("cpu", 12)[0] is tw and engine.weight_luts("cpu")[0].shape == (256,)
    for lib in (nat.hip_lib, nat.host_lib()):
        a8, d8 = np.empty(256), np.empty(256)
        assert lib.hm_gaussian_weight_lut_host(a8.ctypes.data_as(C.POINTER(C.c_double)), d8.ctypes.data_as(C.POINTER(C.c_double))) == 0
        a16, d16 = np.empty(65536), np.empty(65536)
        assert lib.hm_gaussian_weight_lut_bits_host(16, a16.ctypes.data_as(C.POINTER(C.c_double)), d16.ctypes.data_as(C.POINTER(C.c_double))) == 0
        assert np.array_equal(a16[k * 257].view(np.int64), a8.view(np.int64)) and np.array_equal(d16[k * 257].view(np.int64), d8.view(np.int64))
        np.testing.assert_allclose(a16, w16, rtol=1e-15)
        for bad in (7, 17, -1):
            assert lib.hm_gaussian_weight_lut_bits_host(bad, a16.ctypes.data_as(C.POINTER(C.c_double)), None) == nat.HM_EINVAL
        assert lib.hm_gaussian_weight_lut_bits_host(12, None, None) == nat.HM_EINVAL


# ---------------------------------------------------------------------------------------------- dispatch and rules (both libraries, dry)
BASE = 1 << 20


def _args(n=7, C_=3, H=64, W=64, flat=False, sumw=False, variant=0, struct_size=None, out_kind=0, std=False, row0=0, buf_row0=0):
    """Fake, aligned pointers: hm_merge_u16_describe runs the library's own dispatch with launching switched off."""
    from camera_linearity_amd import _native as nat
    a = nat.MergeArgs()
    a.struct_size = C.sizeof(nat.MergeArgs) if struct_size is None else struct_size
    a.n_frames, a.channels, a.variant, a.out_kind = n, C_, variant, out_kind
    a.height, a.width = H, W
    a.row0, a.rows, a.buf_row0, a.buf_rows = row0, H - row0, buf_row0, H - buf_row0
    ex = (C.c_double * n)(*[1e-3 * 1.2 ** i for i in range(n)])
    a.exposures = C.cast(ex, C.POINTER(C.c_double))
    a.icrf, a.w_lut, a.out_val = BASE * 40, BASE * 41, BASE * 42
    a._keep = [ex]
    if std:
        sd = (C.c_void_p * n)(*[BASE * (50 + i) for i in range(n)])
        a.stds = C.cast(sd, C.POINTER(C.c_void_p))
        a.icrf_diff, a.dw_lut, a.out_std = BASE * 43, BASE * 44, BASE * 45
        a._keep.append(sd)
    if flat:
        a.flat_f64, a.flat_std = BASE * 46, BASE * 47
    if sumw:
        a.out_sum_w = BASE * 48
    return a


def _frames(n=7, offset=0):
    return (C.c_void_p * n)(*[BASE * (i + 1) + offset for i in range(n)])


def _describe(lib, a, fr, bits):
    buf = C.create_string_buffer(1024)
    rc = lib.hm_merge_u16_describe(C.byref(a), fr, bits, C.addressof(buf), 1024)
    return rc, buf.value.decode()


S_LDS, S_GLB, GEN = "merge_u16_stream<tab=lds,bits=%d,", "merge_u16_stream<tab=global,bits=%d,", "merge_u16_generic<bits=%d,"
S_MIX = "merge_u16_stream<tab=mixed-%s,bits=%%d,"
# The fit rule, n = 2^b: everything in LDS - value-only 8 (1 + C) n bytes, with std 16 (1 + C) n bytes - where that is at most 160 KiB. The
# largest such depth: C = 3 value-only 12, with std 11; C = 4 value-only 12 (exactly 160 KiB), with std 11 (exactly 160 KiB).
FIT = {(3, False): 12, (3, True): 11, (4, False): 12, (4, True): 11, (1, False): 13, (1, True): 12, (2, False): 12, (2, True): 11}
LDS_MAX = 160 * 1024


def mixed_placement(c, b, std):
    """The largest PARTIAL placement that fits (variant 3): {w, dw} and g, else the per-DN tables alone, else None."""
    n = 2 ** b
    if std and 8 * (2 + c) * n <= LDS_MAX:
        return "mixed-wdwg"
    if (16 if std else 8) * n <= LDS_MAX:
        return "mixed-wdw" if std else "mixed-w"
    return None


def fits_lds(c, b, std):
    return (16 if std else 8) * (1 + c) * 2 ** b <= LDS_MAX


def placement(c, b, std, variant=0):
    """Where hm_merge_u16's streaming kernel keeps its tables, as its name says it (restated from hdrmerge.h)."""
    if variant == 1 or (variant == 0 and fits_lds(c, b, std)):
        return "lds"
    if variant == 2:
        return "global"
    return mixed_placement(c, b, std) or "global"


DISPATCH = [
    (dict(), 12, 0, [S_LDS + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),                              # 12-bit colour value-only: LDS (128 KiB)
    (dict(std=True), 10, 0, [S_LDS + "C=3,std=1,flat=0,sum_w=0>(N=7)"]),                      # 10-bit colour with std: LDS (64 KiB)
    (dict(std=True), 12, 0, [S_MIX % "wdwg" + "C=3,std=1,flat=0,sum_w=0>(N=7)"]),               # 12-bit colour with std: {w, dw} + g in LDS (160 KiB)
    (dict(std=True, C_=4), 12, 0, [S_MIX % "wdw" + "C=4,std=1,flat=0,sum_w=0>(N=7)"]),
    (dict(std=True), 13, 0, [S_MIX % "wdw" + "C=3,std=1,flat=0,sum_w=0>(N=7)"]),
    (dict(std=True), 14, 0, [S_GLB + "C=3,std=1,flat=0,sum_w=0>(N=7)"]),
    (dict(), 14, 0, [S_MIX % "w" + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),
    (dict(), 15, 0, [S_GLB + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),
    (dict(), 16, 0, [S_GLB + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),
    (dict(variant=3), 12, 0, [S_MIX % "w" + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),                  # forced partial placement where everything fits
    (dict(variant=3, std=True), 10, 0, [S_MIX % "wdwg" + "C=3,std=1,flat=0,sum_w=0>(N=7)"]),
    (dict(variant=2, std=True), 12, 0, [S_GLB + "C=3,std=1,flat=0,sum_w=0>(N=7)"]),
    (dict(std=True, flat=True, sumw=True, out_kind=1), 10, 0, [S_LDS + "C=3,std=1,flat=1,sum_w=1,out=f32>(N=7)"]),
    (dict(variant=2), 12, 0, [S_GLB + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),
    (dict(variant=1, std=True), 11, 0, [S_LDS + "C=3,std=1,flat=0,sum_w=0>(N=7)"]),
    (dict(variant=-1), 12, 0, [GEN + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),
    (dict(H=13, W=37), 12, 0, [S_LDS + "C=3,std=0,flat=0,sum_w=0>(N=7)", GEN + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),    # groups + a tail
    (dict(H=1, W=20), 12, 0, [GEN + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),                        # less than one group
    (dict(n=32, C_=1, H=8, W=64, out_kind=1), 9, 0, [S_LDS + "C=1,std=0,flat=0,sum_w=0,out=f32>(N=32)"]),
    # the pair rule: 2- but not 4-byte aligned frames; a row tile with odd W * C at an odd / an even element offset
    (dict(), 12, 2, [GEN + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),
    (dict(H=16, W=37, row0=4, buf_row0=3), 12, 0, [GEN + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),
    (dict(H=16, W=37, row0=5, buf_row0=3), 12, 0, [S_LDS + "C=3,std=0,flat=0,sum_w=0>(N=7)", GEN + "C=3,std=0,flat=0,sum_w=0>(N=7)"]),
]


@pytest.mark.parametrize("kw,bits,offset,names", DISPATCH, ids=[str(i) for i in range(len(DISPATCH))])
def test_dispatch_names(kw, bits, offset, names):
    from camera_linearity_amd import _native as nat
    n = kw.get("n", 7)
    rc, got = _describe(nat.hip_lib, _args(**kw), _frames(n, offset), bits)
    assert rc == nat.HM_OK and got == " + ".join(x.replace("%d", str(bits), 1) if "%d" in x else x for x in names), got
    rc, got = _describe(nat.host_lib(), _args(**kw), _frames(n, offset), bits)
    assert rc == nat.HM_OK and got.startswith("merge_u16_host<") and f"bits={bits}" in got and ("out=f32" in got) == bool(kw.get("out_kind"))


@pytest.mark.parametrize("c,std", sorted(FIT))
def test_fit_rule(c, std):
    """Default dispatch at the largest depth whose tables fit in LDS and at the first that does not; variant 1 there is refused, and every
    depth's default and variant 3 follow the rule as hdrmerge.h states it."""
    from camera_linearity_amd import _native as nat
    b = FIT[(c, std)]
    assert fits_lds(c, b, std) and not fits_lds(c, b + 1, std)
    for depth in range(9, 17):
        assert f"tab={placement(c, depth, std)}," in _describe(nat.hip_lib, _args(C_=c, std=std), _frames(), depth)[1]
        for lib in (nat.hip_lib, nat.host_lib()):
            rc, got = _describe(lib, _args(C_=c, std=std, variant=3), _frames(), depth)
            assert rc == (nat.HM_OK if mixed_placement(c, depth, std) else nat.HM_EUNSUPPORTED)
            assert lib is not nat.hip_lib or rc != nat.HM_OK or f"tab={mixed_placement(c, depth, std)}," in got
    for lib in (nat.hip_lib, nat.host_lib()):
        assert _describe(lib, _args(C_=c, std=std, variant=1), _frames(), b)[0] == nat.HM_OK
        assert _describe(lib, _args(C_=c, std=std, variant=1), _frames(), b + 1)[0] == nat.HM_EUNSUPPORTED
    assert "tab=lds" in _describe(nat.hip_lib, _args(C_=c, std=std), _frames(), b)[1]
    assert "tab=mixed-" in _describe(nat.hip_lib, _args(C_=c, std=std), _frames(), b + 1)[1]
    assert "tab=lds" in _describe(nat.hip_lib, _args(C_=c, std=std, variant=1), _frames(), b)[1]
    assert "tab=global" in _describe(nat.hip_lib, _args(C_=c, std=std, variant=2), _frames(), b)[1]


def test_abi_unchanged_and_symbols():
    from camera_linearity_amd import _native as nat
    assert C.sizeof(nat.MergeArgs) == 296 and nat.hip_lib.hm_version() == 2 and nat.host_lib().hm_version() == 2
    for name in ("hm_merge_u16", "hm_merge_u16_describe", "hm_merge_u16_algorithmic_bytes", "hm_linearize_u16", "hm_gaussian_weight_lut_bits_host"):
        assert name in nat.EXPORTED_SYMBOLS
        for lib in (nat.hip_lib, nat.host_lib()):
            assert callable(getattr(lib, name))


def test_algorithmic_bytes():
    """2 N bytes per element for the frames, the rest as hm_merge: the difference to the uint8 call of the same shape is N per element."""
    from camera_linearity_amd import _native as nat
    for kw in (dict(), dict(std=True), dict(std=True, flat=True, sumw=True), dict(out_kind=1, n=9, C_=4, H=13, W=37, row0=2)):
        a = _args(**kw)
        n = kw.get("n", 7)
        E = (kw.get("H", 64) - kw.get("row0", 0)) * kw.get("W", 64) * kw.get("C_", 3)
        u8 = _args(**kw)
        fr = _frames(n)
        u8.frames_u8 = C.cast(fr, C.POINTER(C.c_void_p))
        for lib in (nat.hip_lib, nat.host_lib()):
            assert lib.hm_merge_u16_algorithmic_bytes(C.byref(a)) - lib.hm_merge_algorithmic_bytes(C.byref(u8)) == n * E
        out = (4 if kw.get("out_kind") else 8) * (2 if kw.get("std") else 1) + (8 if kw.get("sumw") else 0)
        inp = 2 * n + (8 * n if kw.get("std") else 0) + ((16 if kw.get("std") else 8) if kw.get("flat") else 0)
        assert nat.hip_lib.hm_merge_u16_algorithmic_bytes(C.byref(a)) == (inp + out) * E
    assert nat.hip_lib.hm_merge_u16_algorithmic_bytes(None) == 0


@pytest.mark.parametrize("which", ["hip", "host"])
def test_status_codes(which):
    """Every status of the specification, in its order of checks (an earlier rule wins over a later one broken in the same call)."""
    from camera_linearity_amd import _native as nat
    lib = nat.hip_lib if which == "hip" else nat.host_lib()
    buf = C.create_string_buffer(256)

    def rc(a, fr=None, n=7, offset=0, bits=12):
        return lib.hm_merge_u16_describe(C.byref(a), _frames(n, offset) if fr is None else fr, bits, C.addressof(buf), 256)
    # 1. HM_EINVAL
    assert lib.hm_merge_u16(None, 8, 12, None) == nat.HM_EINVAL               # NULL args: before anything else is read
    assert lib.hm_merge_u16_describe(None, 8, 12, C.addressof(buf), 256) == nat.HM_EINVAL
    assert rc(_args()) == nat.HM_OK
    assert rc(_args(struct_size=100), offset=1) == nat.HM_EINVAL
    for field in ("frames_u8", "frames_f64"):
        a = _args()
        fr = _frames()
        setattr(a, field, C.cast(fr, C.POINTER(C.c_void_p)))
        assert rc(a, offset=1) == nat.HM_EINVAL, field                       # (wins over the misaligned frames)
    assert lib.hm_merge_u16_describe(C.byref(_args()), None, 12, C.addressof(buf), 256) == nat.HM_EINVAL
    assert lib.hm_merge_u16(C.byref(_args()), None, 12, None) == nat.HM_EINVAL
    fr = _frames(7, 1)
    fr[6] = None
    assert rc(_args(), fr) == nat.HM_EINVAL                                  # a NULL entry wins over the misaligned ones before it
    for bits in (8, 17, 0, -1):
        assert rc(_args(), offset=1, bits=bits) == nat.HM_EINVAL
    a = _args()
    a.w_lut = None
    assert rc(a, offset=1) == nat.HM_EINVAL
    for field in ("icrf_diff", "dw_lut"):
        a = _args(std=True)
        setattr(a, field, None)
        assert rc(a, offset=1) == nat.HM_EINVAL, field
    # 2. HM_EALIGN: before every remaining rule of hm_merge and before what is unsupported
    assert rc(_args(), offset=1) == nat.HM_EALIGN
    assert lib.hm_merge_u16(C.byref(_args()), _frames(7, 1), 12, None) == nat.HM_EALIGN
    a = _args()
    a.exposures = None
    assert rc(a, offset=1) == nat.HM_EALIGN
    assert rc(_args(n=33), n=33, offset=1) == nat.HM_EALIGN
    assert rc(_args(), offset=2) == nat.HM_OK                                # 2-byte aligned is legal (the generic kernel)
    # 3. hm_merge's rules
    assert rc(a) == nat.HM_EINVAL                                            # no exposures
    assert rc(_args(C_=5)) == nat.HM_EUNSUPPORTED
    assert rc(_args(row0=65)) == nat.HM_EINVAL and rc(_args(H=8, row0=4, buf_row0=5)) == nat.HM_ESHAPE
    a = _args(std=True)
    a.out_std = None
    assert rc(a) == nat.HM_EINVAL
    a = _args()
    a.out_val = BASE * 42 + 4
    assert rc(a) == nat.HM_EALIGN
    a = _args(flat=True, std=True)
    a.flat_std = None
    assert rc(a) == nat.HM_EINVAL
    assert rc(_args(variant=4)) == nat.HM_EINVAL and rc(_args(variant=3)) == nat.HM_OK
    for sz in (264, 280):                                                    # the layouts of ABI version 1
        assert rc(_args(struct_size=sz)) == nat.HM_OK
    a = _args(sumw=True)                                                     # sum of weights only
    a.out_val = None
    assert rc(a) == nat.HM_OK
    # 4. HM_EUNSUPPORTED, before any launch
    a = _args()
    dk = (C.c_void_p * 7)(*[BASE * 90] * 7)
    a.darks_u8 = C.cast(dk, C.POINTER(C.c_void_p))
    assert rc(a) == nat.HM_EINVAL                                            # (hm_merge's rule first: dark maps without thresholds)
    dm = (C.c_int32 * 7)(*[13] * 7)
    a.dark_min_dn, a.median_k = C.cast(dm, C.POINTER(C.c_int32)), 3
    assert rc(a) == nat.HM_EUNSUPPORTED
    assert lib.hm_merge_u16(C.byref(a), _frames(), 12, None) == nat.HM_EUNSUPPORTED
    a = _args()
    a.flat_u8 = BASE * 46
    assert rc(a) == nat.HM_EUNSUPPORTED
    assert rc(_args(n=33), n=33) == nat.HM_EUNSUPPORTED
    assert lib.hm_merge_u16(C.byref(_args(n=33)), _frames(33), 12, None) == nat.HM_EUNSUPPORTED
    for v in (-2, -5):
        assert rc(_args(variant=v)) == nat.HM_EUNSUPPORTED
    assert rc(_args(variant=1), bits=13) == nat.HM_EUNSUPPORTED and rc(_args(variant=1), bits=12) == nat.HM_OK
    assert rc(_args(variant=3), bits=15) == nat.HM_EUNSUPPORTED and rc(_args(variant=3), bits=14) == nat.HM_OK
    # hm_linearize_u16
    for bits in (8, 17):
        assert lib.hm_linearize_u16(BASE, None, BASE * 2, None, BASE * 3, None, None, 10, 3, 3, bits, None) == nat.HM_EINVAL
    assert lib.hm_linearize_u16(BASE, None, BASE * 2, None, BASE * 3, None, None, 10, 3, 2, 12, None) == nat.HM_EINVAL
    assert lib.hm_linearize_u16(BASE + 1, None, BASE * 2, None, BASE * 3, None, None, 10, 3, 3, 12, None) == nat.HM_EALIGN
    assert lib.hm_linearize_u16(BASE, None, BASE * 2, None, BASE * 3, None, BASE * 4 + 1, 10, 3, 3, 12, None) == nat.HM_EALIGN
    assert lib.hm_linearize_u16(BASE, None, BASE * 2, None, BASE * 3, None, None, 0, 3, 3, 12, None) == nat.HM_OK


# ---------------------------------------------------------------------------------------------- Python surface
def test_plan_merge_rules(heng):
    from camera_linearity_amd import _native as nat
    rng = np.random.default_rng(3)
    n, shape, b = 3, (6, 7, 3), 12
    f16 = [T(f) for f in full_range_frames(rng, n, shape, b)]
    f8 = [T(rng.integers(0, 256, size=shape).astype(np.uint8)) for _ in range(n)]
    t = exposures(n)
    icrf, diff = tables_bits(3, b)
    icrf8, diff8 = tables8(3)
    for bad in (None, 8, 17, 12.0, True):
        with pytest.raises(ValueError, match="bit_depth"):
            heng.plan_merge(f16, t, icrf, bit_depth=bad)
    for frames in (f8, [f.double() for f in f8]):
        with pytest.raises(ValueError, match="bit_depth"):
            heng.plan_merge(frames, t, icrf8, bit_depth=12)
    with pytest.raises(ValueError, match="4096"):
        heng.plan_merge(f16, t, icrf8, bit_depth=12)                         # 256-row tables
    with pytest.raises(ValueError, match="4096"):
        heng.plan_merge(f16, t, icrf, diff8, [torch.ones(shape, dtype=F64)] * n, bit_depth=12)
    with pytest.raises(NotImplementedError, match="std_table"):
        heng.plan_merge(f16, t, icrf, diff, std_table=diff, bit_depth=12)
    with pytest.raises(NotImplementedError, match="dark"):
        heng.plan_merge(f16, t, icrf, darks=[None, f8[0], None], dark_min=[256, 3, 256], bit_depth=12)
    with pytest.raises(NotImplementedError, match="uint8 flat"):
        heng.plan_merge(f16, t, icrf, flat=f8[0], ff_mean=[1, 1, 1], bit_depth=12)
    with pytest.raises(NotImplementedError, match=str(nat.HM_MAX_FRAMES)):
        heng.plan_merge([f16[0]] * 33, exposures(33), icrf, bit_depth=12)
    with pytest.raises(NotImplementedError, match=str(nat.HM_MAX_FRAMES)):
        heng.plan_merge(f16, t, icrf, bit_depth=12, variant=-2)
    with pytest.raises(ValueError, match="bit_depth"):
        heng.linearize(f16[0], None, icrf)
    with pytest.raises(ValueError, match="bit_depth"):
        heng.linearize(f8[0], None, icrf8, bit_depth=12)
    with pytest.raises(ValueError, match="4096"):
        heng.linearize(f16[0], None, icrf8, bit_depth=12)
    # bit_depth = None: unchanged
    p8 = heng.plan_merge(f8, t, icrf8)
    assert p8._entry == "hm_merge" and p8.bit_depth is None and p8.args.frames_u8
    # a uint16 plan goes through hm_merge_u16 with the frames beside the struct; float32 stds are widened
    lib = nat.host_lib()
    calls = lib.calls["hm_merge_u16"]
    sd32 = [T(s.astype(np.float32)) for s in make_stds(rng, n, shape)]
    p = heng.plan_merge(f16, t, icrf, diff, sd32, bit_depth=12)
    assert p._entry == "hm_merge_u16" and p.bit_depth == 12 and not p.args.frames_u8 and not p.args.frames_f64 and p.args.stds
    assert "f32" not in p.kernels
    p.launch()
    assert lib.calls["hm_merge_u16"] == calls + 1
    want = heng.merge(f16, t, icrf, diff, [s.double() for s in sd32], bit_depth=12)
    for k in want:
        assert_same_bits(p.outputs[k], want[k], k)
    assert p.algorithmic_bytes == (2 * n + 8 * n + 16) * int(np.prod(shape))


def test_tiff_round_trip_into_plan_merge(heng, tmp_path):
    """uint16 frames written and read back by tiff_io go into plan_merge(bit_depth=12) as they come."""
    from camera_linearity_amd import tiff_io
    rng = np.random.default_rng(8)
    n, shape, b = 3, (9, 11, 3), 12
    frames = full_range_frames(rng, n, shape, b)
    back = []
    for i, f in enumerate(frames):
        assert tiff_io.imwrite(tmp_path / f"f{i}.tif", f)
        r = tiff_io.imread(tmp_path / f"f{i}.tif", tiff_io.IMREAD_UNCHANGED)
        assert r.dtype == np.uint16 and np.array_equal(r, f)
        back.append(T(r))
    icrf, diff = tables_bits(3, b)
    got = heng.merge(back, exposures(n), icrf, bit_depth=b)
    want = numpy_merge_u16(frames, b, exposures(n), icrf)
    np.testing.assert_allclose(got["val"].numpy(), want["val"], rtol=VAL_RTOL, atol=0)
