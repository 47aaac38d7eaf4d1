"""The fused merge reading float32 std frames as they are (engine.plan_merge with torch.float32 stds, hm_merge_std_f32) on the MI355X.

Exact criterion, no tolerance: widening float32 to float64 loses nothing, so the float32-std plan's outputs equal those of the same plan
fed [s.to(torch.float64) for s in stds32], compared as integer bit patterns (NaN positions must coincide) - and both equal the generic
kernel (variant = -1). Every case asserts through plan.kernels which kernel family ran and that every part that reads stds carries
"std=f32", and that algorithmic_bytes differs from the float64-std plan's by exactly 4 N numel.
Stds: random float32 * 0.02 with about 5 % exact zeros, one subnormal (1e-45), one 3e38 and - only in cases without dark maps, a median
of NaNs has no defined answer - one +inf and one NaN."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import hdr_oracle as orc  # noqa: E402

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from camera_linearity_amd import engine
    return engine


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def assert_same_bits(a, b, what=""):
    """NaN positions coincide, every other element has the same bit pattern."""
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), what
    it = torch.int64 if a.dtype == F64 else torch.int32
    assert torch.equal(a.contiguous().view(it)[~na], b.contiguous().view(it)[~nb]), what


def same_bits(out32, out64, what=""):
    """The rule of tests/test_gpu_merge_f32.py: float32 output == NumPy's conversion of the float64 output."""
    a, b = out64.cpu().numpy(), out32.cpu().numpy()
    assert a.dtype == np.float64 and b.dtype == np.float32 and a.shape == b.shape, (what, a.dtype, b.dtype)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        want = a.astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(b)), what
    bad = want.view(np.int32)[~nan] != b.view(np.int32)[~nan]
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8])


def make_stds(seed, n, shape, nonfinite=True):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s = rng.random(shape, dtype=np.float32) * np.float32(0.02)
        s[rng.random(shape) < 0.05] = 0.0
        out.append(s)
    flat = out[0].reshape(-1)                              # (in the first frames: every sub-stack of the shared fixture sees them)
    flat[1] = np.float32(1e-45)                            # the smallest float32 subnormal
    out[min(1, n - 1)].reshape(-1)[2] = np.float32(3e38)
    if nonfinite:
        flat[3] = np.inf
        out[min(2, n - 1)].reshape(-1)[7] = np.nan
    return out


def f32_vs_f64(eng, fr, t, icrf, diff, sd32, expect=(), absent=(), **kw):
    """The float32-std plan against the float64-std plan of the widened frames; `expect`: substrings its kernels must hold. -> its outputs."""
    assert all(s.dtype == F32 for s in sd32)
    p64 = eng.plan_merge(fr, t, icrf, diff, [s.to(F64) for s in sd32], **kw)
    p32 = eng.plan_merge(fr, t, icrf, diff, sd32, **kw)
    names = p32.kernels
    for e in expect:
        assert e in names, (e, names)
    for e in absent:
        assert e not in names, (e, names)
    for part in names.split(" + "):
        assert "std=f32" in part or part == "merge_scan_hot", names
    assert "std=f32" not in p64.kernels
    for v in p32.outputs.values():
        v.fill_(float("nan"))
    p64.launch()
    p32.launch()
    torch.cuda.synchronize()
    assert p64.outputs.keys() == p32.outputs.keys() and "std" in p32.outputs
    for k in p64.outputs:
        assert_same_bits(p32.outputs[k], p64.outputs[k], (k, names))
    assert p64.algorithmic_bytes - p32.algorithmic_bytes == 4 * len(fr) * p32.outputs["val"].numel()
    return p32.outputs


@pytest.fixture(scope="module")
def stack(eng):
    """96 x 130 x 3, 33 frames with float32 stds and a flat field - made once, never written."""
    h, w = 96, 130
    frames, _, t = orc.synthetic_stack(700, 33, h, w)
    icrf, diff = orc.synthetic_icrf()
    rng = np.random.default_rng(700)
    flat = rng.integers(180, 230, size=(h, w, 3)).astype(np.uint8)
    return dict(fr=[dev(f) for f in frames], sd=[dev(s) for s in make_stds(700, 33, (h, w, 3))], t=list(t), icrf=icrf, diff=diff, flat=dev(flat),
                flat_std=dev(np.full((h, w, 3), 0.002)), ff_mean=[0.8, 0.81, 0.79], ff_std_mean=[0.002] * 3, h=h, w=w)


def take(stack, n):
    return stack["fr"][:n], stack["sd"][:n], stack["t"][:n]


def flat_kw(s):
    return dict(flat=s["flat"], ff_mean=s["ff_mean"], flat_std=s["flat_std"], ff_std_mean=s["ff_std_mean"])


def family(n, flat, sumw):
    if n in (7, 15) and not sumw:
        return f"merge_u8_fast_std<N={n},U=1,flat={int(flat)},sum_w=0,std=f32"
    return f"merge_u8_loop_std<C=3,flat={int(flat)},sum_w={int(sumw)},std=f32"


# ---- 1
@pytest.mark.parametrize("sumw", [False, True])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("n", [1, 7, 8, 15, 16, 17, 20, 21, 32])
def test_f32_stds_96x130(eng, stack, n, flat, sumw):
    """37 440 elements: whole groups, a generic tail, more than one workgroup. N = 7 and 15 take the compile-time-N kernel (without a
    sum-of-weights output), everything else merge_u8_loop_std; float64 and float32 outputs; the generic kernel gives the same bits."""
    s = stack
    kw = dict(flat_kw(s) if flat else {}, **(dict(want_sum_w=True) if sumw else {}))
    fr, sd, t = take(s, n)
    fam = family(n, flat, sumw)
    out = f32_vs_f64(eng, fr, t, s["icrf"], s["diff"], sd, expect=[fam + ">", "merge_generic<f64in=0,std=1,std=f32>"], **kw)
    assert not torch.isfinite(out["std"]).all() and float((out["std"] > 0).double().mean()) > 0.5
    gen = f32_vs_f64(eng, fr, t, s["icrf"], s["diff"], sd, expect=["merge_generic<f64in=0,std=1,std=f32>"], absent=["merge_u8"], variant=-1, **kw)
    for k in out:
        assert_same_bits(out[k], gen[k], k)
    o32 = f32_vs_f64(eng, fr, t, s["icrf"], s["diff"], sd, expect=[fam + ",out=f32>"], out_dtype=F32, **kw)
    for k in ("val", "std"):
        same_bits(o32[k], out[k], k)


# ---- 2
def _raw_call(nat, plan, ptrs):
    """hm_merge_std_f32 on a plan's argument struct with args->stds cleared and `ptrs` as the float32 std frames."""
    a = plan.args
    a.stds = C.POINTER(C.c_void_p)()
    arr = (C.c_void_p * len(ptrs))(*ptrs)
    st = torch.cuda.current_stream().cuda_stream
    rc = nat.hip_lib.hm_merge_std_f32(C.byref(a), arr, st)
    torch.cuda.synchronize()
    return rc


def test_f32_fallbacks_widen(eng, stack):
    """33 frames and a forced chunking: the plan widens, as before (no "std=f32", the same results as float64 stds); called directly,
    hm_merge_std_f32 refuses both before any launch and leaves the outputs alone."""
    from camera_linearity_amd import _native as nat
    s = stack
    for n, variant in ((33, 0), (7, -2)):
        fr, sd, t = take(s, n)
        p = eng.plan_merge(fr, t, s["icrf"], s["diff"], sd, variant=variant)
        assert "f32" not in p.kernels and p.args.stds
        want = eng.merge(fr, t, s["icrf"], s["diff"], [x.to(F64) for x in sd], variant=variant)
        p.launch()
        torch.cuda.synchronize()
        for k in want:
            assert_same_bits(p.outputs[k], want[k], (n, variant, k))
        if n <= 32:
            one = eng.merge(fr, t, s["icrf"], s["diff"], sd)
            for k in want:
                assert_same_bits(one[k], want[k], k)
        for v in p.outputs.values():
            v.fill_(float("nan"))
        torch.cuda.synchronize()
        assert _raw_call(nat, p, [x.data_ptr() for x in sd]) == nat.HM_EUNSUPPORTED
        assert all(bool(torch.isnan(v).all()) for v in p.outputs.values())


# ---- 3
@pytest.mark.parametrize("Cc", [1, 2, 4])
def test_f32_other_channel_counts(eng, Cc):
    n, h, w = 7, 40, 52
    frames, _, t = orc.synthetic_stack(710 + Cc, n, h, w, c=Cc)
    icrf = np.stack([np.linspace(0, 1, 256) ** (1.5 + 0.2 * k) for k in range(Cc)], axis=1)
    diff = orc.icrf_derivative(icrf)
    fr, sd = [dev(f) for f in frames], [dev(x) for x in make_stds(710 + Cc, n, (h, w, Cc))]
    rng = np.random.default_rng(Cc)
    kw = dict(flat=dev(rng.integers(180, 230, size=(h, w, Cc)).astype(np.uint8)), ff_mean=[0.8, 0.81, 0.79, 0.82][:Cc], want_sum_w=True,
              flat_std=dev(np.full((h, w, Cc), 0.002)), ff_std_mean=[0.002] * Cc)
    a = f32_vs_f64(eng, fr, list(t), icrf, diff, sd, expect=[f"merge_u8_loop_std<C={Cc},flat=0,sum_w=0,std=f32>(N=7)"])
    b = f32_vs_f64(eng, fr, list(t), icrf, diff, sd, expect=[f"merge_u8_loop_std<C={Cc},flat=1,sum_w=1,std=f32>(N=7)"], **kw)
    c = f32_vs_f64(eng, fr, list(t), icrf, diff, sd, expect=[f"merge_u8_loop_std<C={Cc},flat=1,sum_w=1,std=f32,out=f32>(N=7)"], out_dtype=F32, **kw)
    same_bits(c["std"], b["std"])
    for out, k2 in ((a, {}), (b, kw)):
        gen = f32_vs_f64(eng, fr, list(t), icrf, diff, sd, expect=["merge_generic"], absent=["merge_u8"], variant=-1, **k2)
        for k in out:
            assert_same_bits(out[k], gen[k], k)


# ---- 4
def test_f32_float64_frames(eng):
    n, h, w = 5, 40, 52
    frames, _, t = orc.synthetic_stack(720, n, h, w)
    rng = np.random.default_rng(720)
    f64 = []
    for f in frames:
        v = (f.astype(np.float64) + rng.choice([0.0, 0.5, 0.25, -0.25], size=f.shape)) / 255.0
        v[rng.random(f.shape) < 0.05] += 1.0
        f64.append(dev(v))
    icrf, diff = orc.synthetic_icrf()
    sd = [dev(x) for x in make_stds(720, n, (h, w, 3))]
    out = f32_vs_f64(eng, f64, list(t), icrf, diff, sd, expect=["merge_generic<f64in=1,std=1,std=f32>"], absent=["merge_f64"])
    o32 = f32_vs_f64(eng, f64, list(t), icrf, diff, sd, expect=["merge_generic<f64in=1,std=1,std=f32,out=f32>"], out_dtype=F32)
    same_bits(o32["std"], out["std"])
    d = rng.integers(0, 10, size=(h, w, 3)).astype(np.uint8)
    d[rng.random(d.shape) < 0.02] = 200
    sd = [dev(x) for x in make_stds(721, n, (h, w, 3), nonfinite=False)]
    for hq in (True, False):
        f32_vs_f64(eng, f64, list(t), icrf, diff, sd, darks=[dev(d)] * n, dark_min=[100] * n, median_k=3, hot_queue=hq,
                   expect=["merge_patch_hot<f64in=1,std=1,std=f32>" if hq else "merge_fixup_hot<f64in=1,std=1,std=f32>"])


# ---- 5
def _dark_case(seed, density=0.01):
    n, h, w = 7, 64, 64
    rng = np.random.default_rng(seed)
    _, _, t = orc.synthetic_stack(seed, n, 4, 4)
    frames = [rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8) for _ in range(n)]
    d = rng.integers(0, 10, size=(h, w, 3)).astype(np.uint8)
    d[rng.random(d.shape) < density] = 200
    for y, x, c in ((0, 0, 0), (0, w - 1, 1), (h - 1, 0, 2), (h - 1, w - 1, 0), (31, 0, 1), (32, w - 1, 2)):
        d[y, x, c] = 255                                   # hot pixels on the image border: reflect
    d.reshape(-1)[1000:1050] = 255
    return n, h, w, frames, list(t), d, make_stds(seed, n, (h, w, 3), nonfinite=False)


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("hot_queue", [True, False])
def test_f32_dark_maps(eng, hot_queue, k):
    """One map for every frame (each hot element is hot in two and more frames at once), then one frame without a map; the std of a hot
    frame is the median of its float32 neighbourhood."""
    n, h, w, frames, t, d, sd = _dark_case(740)
    icrf, diff = orc.synthetic_icrf()
    fr, dk, sd = [dev(f) for f in frames], dev(d), [dev(x) for x in sd]
    expect = ["merge_scan_hot + merge_patch_hot<f64in=0,std=1,std=f32>"] if hot_queue else ["merge_fixup_hot<f64in=0,std=1,std=f32>"]
    out = f32_vs_f64(eng, fr, t, icrf, diff, sd, darks=[dk] * n, dark_min=[100] * n, median_k=k, hot_queue=hot_queue, expect=expect)
    plain = eng.merge(fr, t, icrf, diff, sd)
    assert not torch.equal(out["std"], plain["std"]) and not torch.isnan(out["std"]).any()         # the medians changed something
    gen = f32_vs_f64(eng, fr, t, icrf, diff, sd, darks=[dk] * n, dark_min=[100] * n, median_k=k, hot_queue=hot_queue, variant=-1)
    for key in out:
        assert_same_bits(out[key], gen[key], key)
    o32 = f32_vs_f64(eng, fr, t, icrf, diff, sd, darks=[None] + [dk] * (n - 1), dark_min=[256] + [100] * (n - 1), median_k=k,
                     hot_queue=hot_queue, want_sum_w=True, out_dtype=F32)
    assert o32["std"].dtype == F32


def test_f32_dark_maps_smallest_workspace(eng):
    """A dense map overflows the smallest legal workspace: merge_patch_hot goes over the whole tile."""
    from camera_linearity_amd import _native as nat
    n, h, w, frames, t, d, sd = _dark_case(741, density=0.02)
    icrf, diff = orc.synthetic_icrf()
    fr, dk, sd = [dev(f) for f in frames], dev(d), [dev(x) for x in sd]
    want = eng.merge(fr, t, icrf, diff, [x.to(F64) for x in sd], darks=[dk] * n, dark_min=[100] * n, median_k=3)
    least = int(nat.lib.hm_merge_hot_workspace_min_bytes(h * w * 3))
    p = eng.plan_merge(fr, t, icrf, diff, sd, darks=[dk] * n, dark_min=[100] * n, median_k=3)
    small = torch.zeros(least + 16, dtype=torch.uint8, device="cuda")
    p._keep.append(small)
    p.args.hot_workspace, p.args.hot_workspace_bytes = small.data_ptr(), least
    assert "merge_scan_hot + merge_patch_hot<f64in=0,std=1,std=f32>" in p.kernels
    p.launch()
    torch.cuda.synchronize()
    words = small.cpu().numpy()[:16].view(np.uint32)
    assert words[0] >= 1 and words[1] == 1                 # something was queued, then the one-entry queue overflowed
    for k in ("val", "std"):
        assert_same_bits(p.outputs[k], want[k], k)


# ---- 6
def _offset_views(sd):
    """Views that start one float32 into their allocation: 4- but not 8-byte aligned."""
    out = []
    for s in sd:
        base = torch.empty(s.numel() + 1, dtype=F32, device=s.device)
        base[1:] = s.reshape(-1)
        out.append(base[1:].view(s.shape))
    assert all(v.data_ptr() % 8 == 4 and v.is_contiguous() for v in out)
    return out


def test_f32_alignment_fallbacks(eng, stack):
    from camera_linearity_amd import _native as nat
    s = stack
    fr, sd, t = take(s, 7)
    want = f32_vs_f64(eng, fr, t, s["icrf"], s["diff"], sd, expect=["merge_u8_fast_std"])
    views = _offset_views(sd)
    p = eng.plan_merge(fr, t, s["icrf"], s["diff"], views)
    assert p.kernels == "merge_generic<f64in=0,std=1,std=f32>"
    got = f32_vs_f64(eng, fr, t, s["icrf"], s["diff"], views, expect=["merge_generic<f64in=0,std=1,std=f32>"], absent=["merge_u8"])
    for k in want:
        assert_same_bits(got[k], want[k], k)
    # a row tile with odd W * C and an odd halo: the first input element sits at an odd element offset
    n, h, w = 20, 11, 5
    frames, _, t2 = orc.synthetic_stack(750, n, h, w)
    f2, s2 = [dev(f) for f in frames], [dev(x) for x in make_stds(750, n, (h, w, 3))]
    whole = f32_vs_f64(eng, f2, list(t2), s["icrf"], s["diff"], s2)
    for r0, r1 in ((1, 4), (3, 11), (10, 11)):
        part = f32_vs_f64(eng, f2, list(t2), s["icrf"], s["diff"], s2, expect=["merge_generic<f64in=0,std=1,std=f32>"], absent=["merge_u8"],
                          height=h, row0=r0, rows=r1 - r0)
        for k in ("val", "std"):
            assert_same_bits(part[k], whole[k][r0:r1], (r0, r1, k))
    # 2-byte-misaligned std pointers through the raw ABI
    for v in p.outputs.values():
        v.fill_(float("nan"))
    assert _raw_call(nat, p, [x.data_ptr() + 2 for x in sd]) == nat.HM_EALIGN
    assert all(bool(torch.isnan(v).all()) for v in p.outputs.values())
    assert _raw_call(nat, p, [x.data_ptr() for x in views]) == nat.HM_OK
    for k in want:
        assert_same_bits(p.outputs[k], want[k], k)


# ---- 7
def test_f32_row_tiles_with_median_halo(eng):
    """3 tiles of a 67-row image with dark maps (buf_row0 halo) equal the whole-image call."""
    icrf, diff = orc.synthetic_icrf()
    n, h, w = 7, 67, 130
    frames, _, t = orc.synthetic_stack(731, n, h, w)
    rng = np.random.default_rng(731)
    d = rng.integers(0, 30, size=(h, w, 3)).astype(np.uint8)
    d[0, 0, 0] = d[h - 1, w - 1, 2] = d[22, 5, 1] = d[23, 5, 1] = d[44, 9, 0] = d[45, 9, 0] = 255      # hot on both sides of the seams
    fr, dk = [dev(f) for f in frames], [None, None] + [dev(d)] * (n - 2)
    sd = [dev(x) for x in make_stds(731, n, (h, w, 3), nonfinite=False)]
    mins = [256, 256] + [20] * (n - 2)
    whole = f32_vs_f64(eng, fr, list(t), icrf, diff, sd, darks=dk, dark_min=mins, median_k=3)
    for r0, r1 in ((0, 23), (23, 45), (45, 67)):
        b0, b1 = max(0, r0 - 1), min(h, r1 + 1)
        part = f32_vs_f64(eng, [f[b0:b1] for f in fr], list(t), icrf, diff, [x[b0:b1] for x in sd], darks=[None if x is None else x[b0:b1] for x in dk],
                          dark_min=mins, median_k=3, height=h, row0=r0, rows=r1 - r0, buf_row0=b0)
        for k in part:
            assert_same_bits(part[k], whole[k][r0:r1], (r0, k))


# ---- 8
@pytest.mark.parametrize("n,flat", [(7, False), (7, True), (20, False)])
def test_f32_steady_state(eng, n, flat):
    """Every wave in its steady state (prefetch, loop back-edge): the streaming launches cap their grid at 8 workgroups of 4 waves per CU
    (launch_one: 2048 / 256 threads, LDS allows more; launch_loop_c: stream_grid(groups, 4, 8)) and a wave takes one 128-element group per
    iteration, so every wave handles more than one group from 2 * 8 * 4 * CUs groups on: 16 384 groups = 2 097 152 elements on the 256 CUs
    of an MI355X - R x 1024 x 3 with R = ceil(16 384 * 128 / 3072) = 683 rows. Against the float64-std plan and variant = -1."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = 2 * 8 * 4 * cus
    w = 1024
    h = -(-groups * 128 // (w * 3))
    assert h * w * 3 // 128 >= groups
    g = torch.Generator(device="cuda").manual_seed(760 + n)
    fr = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(n)]
    sd = [torch.rand((h, w, 3), dtype=F32, device="cuda", generator=g) * 0.02 for _ in range(n)]
    for x in sd:
        x[torch.rand(x.shape, device="cuda", generator=g) < 0.05] = 0.0
    sd[0].view(-1)[1] = 1e-45
    sd[-1].view(-1)[-2] = 3e38
    sd[0].view(-1)[h * w * 3 // 2] = float("inf")
    sd[n // 2].view(-1)[h * w * 3 // 2 + 1001] = float("nan")
    icrf, diff = orc.synthetic_icrf()
    t = list(1e-3 * 1.3 ** np.arange(n))
    kw = {}
    if flat:
        kw = dict(flat=torch.randint(180, 230, (h, w, 3), dtype=torch.uint8, device="cuda", generator=g), ff_mean=[0.8, 0.81, 0.79],
                  flat_std=torch.full((h, w, 3), 0.002, dtype=F64, device="cuda"), ff_std_mean=[0.002] * 3)
    out = f32_vs_f64(eng, fr, t, icrf, diff, sd, expect=[family(n, flat, False) + ">"], **kw)
    gen = eng.plan_merge(fr, t, icrf, diff, sd, variant=-1, **kw)
    assert gen.kernels == "merge_generic<f64in=0,std=1,std=f32>"
    gen.launch()
    torch.cuda.synchronize()
    for k in out:
        assert_same_bits(out[k], gen.outputs[k], k)


# ---- 9
def test_f32_graph_replay(eng, stack):
    """A PlanGraph of float32-std plans replays to the bits of eager launches, twice, with the inputs refreshed in between."""
    s = stack
    f7, sd7, t7 = take(s, 7)
    f21, sd21, t21 = take(s, 21)
    in7, in21 = [x.clone() for x in sd7], [x.clone() for x in sd21]
    p1 = eng.plan_merge(f7, t7, s["icrf"], s["diff"], in7)
    p2 = eng.plan_merge(f21, t21, s["icrf"], s["diff"], in21, out_dtype=F32, **flat_kw(s))
    assert "merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,std=f32>" in p1.kernels and "merge_u8_loop_std<C=3,flat=1,sum_w=0,std=f32,out=f32>(N=21)" in p2.kernels
    graph = eng.PlanGraph([p1, p2])
    for rnd in range(2):
        if rnd:                                             # refreshed inputs: the frames' stds in another order
            for dst, src in zip(in7, reversed(sd7)):
                dst.copy_(src)
            for dst, src in zip(in21, reversed(sd21)):
                dst.copy_(src)
        for p in (p1, p2):
            p.launch()
        torch.cuda.synchronize()
        want = [{k: v.clone() for k, v in p.outputs.items()} for p in (p1, p2)]
        for p in (p1, p2):
            for v in p.outputs.values():
                v.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for p, w_ in zip((p1, p2), want):
            for k in w_:
                assert_same_bits(p.outputs[k], w_[k], (rnd, k))
    e = eng.merge(f7, t7, s["icrf"], s["diff"], [x.to(F64) for x in reversed(sd7)])
    for k in e:
        assert_same_bits(p1.outputs[k], e[k], k)


# ---- 10
def test_f32_merge_pipeline(eng):
    from camera_linearity_amd.pipeline import MergePipeline
    n, h, w = 7, 64, 96
    icrf, diff = orc.synthetic_icrf()
    stacks, stds = [], []
    for k in range(5):
        frames, _, t = orc.synthetic_stack(770 + k, n, h, w)
        stacks.append(frames)
        stds.append(make_stds(770 + k, n, (h, w, 3)))
    pipe = MergePipeline(n, h, w, t, icrf, diff, with_std=True, std_dtype=F32)
    for slot in pipe.slots:
        assert all(x.dtype == F32 and x.is_pinned() for x in slot.h_stds) and all(x.dtype == F32 for x in slot.d_stds)
        assert "merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,std=f32>" in slot.plan.kernels
    assert all(v.dtype == np.float32 for v in pipe.input_views(0)[1])
    got = pipe.merge_many(stacks, stds)
    assert len(got) == 5
    for frames, sd, (val, std) in zip(stacks, stds, got):
        want = eng.merge([dev(f) for f in frames], list(t), icrf, diff, [dev(x) for x in sd])
        wv, ws = want["val"].cpu().numpy(), want["std"].cpu().numpy()
        assert np.array_equal(val.view(np.int64), wv.view(np.int64))
        nan = np.isnan(ws)
        assert np.array_equal(nan, np.isnan(std)) and np.array_equal(std.view(np.int64)[~nan], ws.view(np.int64)[~nan])
    wide = MergePipeline(n, h, w, t, icrf, diff, with_std=True)                          # the default stays float64
    assert all(v.dtype == np.float64 for v in wide.input_views(0)[1]) and "f32" not in wide.slots[0].plan.kernels
    with pytest.raises(ValueError):
        MergePipeline(n, h, w, t, icrf, diff, with_std=True, std_dtype=torch.float16)
    with pytest.raises(ValueError):
        MergePipeline(n, h, w, t, icrf, diff, std_table=np.zeros((256, 3)), std_dtype=F32)


# ---- 11
def _features(t):
    return {"illumination": "bf", "magnification": "5x", "exposure": float(t), "subject": "s"}


def test_f32_process_hdr_image_from_save_32bit_files(eng, tmp_path, monkeypatch):
    """save_32bit writes a stack's stds; from_dir_path(..., use_cupy=True).process_HDR_image(...) loads them as float32 and merges them as
    they are: the merge of the same stds widened, bit for bit, through a plan that names std=f32."""
    from camera_linearity_amd import _native as nat
    from camera_linearity_amd import tiff_io
    from camera_linearity_amd.exposure_series import ExposureSeries
    from camera_linearity_amd.image_set import ImageSet
    n, h, w = 5, 48, 40
    frames, _, t = orc.synthetic_stack(780, n, h, w)
    icrf, diff = orc.synthetic_icrf()
    sd = make_stds(780, n, (h, w, 3), nonfinite=False)
    for f, s_, ti in zip(frames, sd, t):
        path = tmp_path / f"{ti * 1000:g}ms bf 5x sample.tif"
        ImageSet(value=f, std=s_, features=_features(ti), use_cupy=True).save_32bit(save_path=path)
        assert tiff_io.imread(str(path).removesuffix(".tif") + " STD.tif", tiff_io.IMREAD_UNCHANGED).dtype == np.float32
        tiff_io.imwrite(path, f)                            # (save_32bit wrote the value image as float32 under this name: the DNs instead)
    plans = []
    real = eng.plan_merge

    def spy(*a, **kw):
        plans.append(real(*a, **kw))
        return plans[-1]
    monkeypatch.setattr(eng, "plan_merge", spy)
    (series,) = ExposureSeries.from_dir_path(tmp_path, use_cupy=True)
    calls = nat.hip_lib.calls["hm_merge_std_f32"]
    series.process_HDR_image(icrf, diff, dark_list=[], flat_list=[])
    assert nat.hip_lib.calls["hm_merge_std_f32"] == calls + 1
    assert len(plans) == 1 and "merge_u8_loop_std<C=3,flat=0,sum_w=0,std=f32>(N=5)" in plans[0].kernels
    got = series.merged_image_set.measurand
    order = np.argsort(t)
    want = eng.merge([dev(frames[i]) for i in order], [float(t[i]) for i in order], icrf, diff, [dev(sd[i]).to(F64) for i in order])
    assert got.val.is_cuda
    assert_same_bits(got.val, want["val"], "val")
    assert_same_bits(got.std, want["std"], "std")
