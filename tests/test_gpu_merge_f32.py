"""float32 outputs of the fused merge on the MI355X (engine.plan_merge(out_dtype=torch.float32), hm_merge_args.out_kind = HM_OUT_F32).

Exact criterion, no tolerance: the kernels compute in float64 and round once (to nearest even) at the store, so the float32 output of a call
equals the NumPy conversion - done on the host - of the float64 output of the same call: NaNs at the same positions, every other element
bit-identical as int32 (signed zeros, infinities, float32 subnormals). sum_w stays float64 and is bit-identical. The float64 outputs are
pinned to the oracle and the reference's vectors by tests/test_gpu_merge.py. Every case asserts through plan.kernels which kernel family ran."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import hdr_oracle as orc  # noqa: E402

F32 = torch.float32
F32_MAX = float(np.finfo(np.float32).max)
F32_TINY = float(np.finfo(np.float32).tiny)
F32_DENORM_MIN = 2.0 ** -149


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from camera_linearity_amd import engine
    return engine


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def same_bits(out32, out64, what=""):
    a, b = out64.cpu().numpy(), out32.cpu().numpy()
    assert a.dtype == np.float64 and b.dtype == np.float32 and a.shape == b.shape, (what, a.dtype, b.dtype)
    with np.errstate(over="ignore", under="ignore"):
        want = a.astype(np.float32)                       # the conversion is NumPy's, on the host
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(b)), what
    bad = want.view(np.int32)[~nan] != b.view(np.int32)[~nan]
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8])


def both(eng, fr, t, icrf, diff, sd=None, expect=(), **kw):
    """The same call with float64 and float32 outputs; `expect`: substrings plan.kernels of the float32 plan must hold. -> (out64, out32)."""
    kw64 = dict(kw)
    if kw64.get("variant") == 32:                          # (variant 32 exists for float32 calls only: the pair-store form of merge_u8_val3)
        kw64["variant"] = 0
    p64 = eng.plan_merge(fr, t, icrf, diff if sd is not None else None, sd, **kw64)
    p32 = eng.plan_merge(fr, t, icrf, diff if sd is not None else None, sd, out_dtype=F32, **kw)
    names = p32.kernels
    for e in expect:
        assert e in names, (e, names)
    for part in names.split(" + "):
        assert "out=f32" in part or part == "merge_scan_hot", names
    assert "out=" not in p64.kernels
    for v in p32.outputs.values():
        v.fill_(float("nan"))
    p64.launch()
    p32.launch()
    torch.cuda.synchronize()
    assert p64.outputs.keys() == p32.outputs.keys()
    for k in p64.outputs:
        if k == "sum_w":
            assert p32.outputs[k].dtype == torch.float64 and torch.equal(p32.outputs[k], p64.outputs[k])
        else:
            same_bits(p32.outputs[k], p64.outputs[k], (k, names))
    n_out = p64.outputs["val"].numel() * (2 if "std" in p64.outputs else 1) if "val" in p64.outputs else 0
    assert p64.algorithmic_bytes - p32.algorithmic_bytes == 4 * n_out
    return p64.outputs, p32.outputs


@pytest.fixture(scope="module")
def stack():
    """96 x 130 x 3, 32 frames with std, flat field and the tables - uploaded once, never written. A case with n frames takes the n
    frames around the middle one (take()): the synthetic stack exposes its middle frame well, its first frames are black."""
    h, w = 96, 130
    frames, stds, t = orc.synthetic_stack(500, 32, h, w, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    rng = np.random.default_rng(500)
    flat = rng.integers(180, 230, size=(h, w, 3)).astype(np.uint8)
    return dict(fr=[dev(f) for f in frames], sd=[dev(s) for s in stds], t=list(t), icrf=icrf, diff=diff, flat=dev(flat),
                flat_std=dev(np.full((h, w, 3), 0.002)), ff_mean=[0.8, 0.81, 0.79], ff_std_mean=[0.002] * 3, h=h, w=w)


def take(stack, n):
    """(frames, stds, exposures) of the n frames centred on the stack's middle frame."""
    lo = max(0, min(16 - n // 2, 32 - n))
    fr = stack["fr"][lo:lo + n]
    assert all(0 < float((f > 0).float().mean()) for f in fr[n // 2:])          # not a stack of black frames
    return fr, stack["sd"][lo:lo + n], stack["t"][lo:lo + n]


CASES_96 = {
    # name: (n, with_std, flat, sum_w, kernel family the float32 plan must name)
    "n7_val": (7, False, False, False, "merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32x4>"),
    "n7_std": (7, True, False, False, "merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,out=f32>"),
    "n7_flat": (7, False, True, False, "merge_u8_val3<N=7,U=2,PF=1,MAP=3,flat=1,out=f32x4>"),
    "n7_flat_sumw": (7, False, True, True, "merge_u8_fast<N=7,U=2,flat=1,sum_w=1,out=f32>"),
    "n7_flat_sumw_std": (7, True, True, True, "merge_u8_fast_std<N=7,U=1,flat=1,sum_w=1,out=f32>"),
    "n15_val": (15, False, False, False, "merge_u8_val3<N=15,U=3,PF=0,MAP=0,out=f32>"),
    "n15_std": (15, True, False, False, "merge_u8_fast_std<N=15,U=1,flat=0,sum_w=0,out=f32>"),
    "n15_flat": (15, False, True, False, "merge_u8_val3<N=15,U=2,PF=1,MAP=0,flat=1,out=f32x4>"),
    "n20_std": (20, True, False, False, "merge_u8_loop_std<C=3,flat=0,sum_w=0,out=f32>(N=20)"),
    "n21_std": (21, True, False, False, "merge_u8_loop_std<C=3,flat=0,sum_w=0,out=f32>(N=21)"),
    "n32_std": (32, True, False, False, "merge_u8_loop_std<C=3,flat=0,sum_w=0,out=f32>(N=32)"),
    "n21_val": (21, False, False, False, "merge_u8_loop<C=3,flat=0,sum_w=0,out=f32>(N=21)"),
}


@pytest.mark.parametrize("name", list(CASES_96))
def test_f32_equals_cast_96x130(eng, stack, name):
    """Every streaming family at 96 x 130 x 3 = 37 440 elements (73 units of 512 + a generic tail; more than one workgroup), and the generic
    kernel (variant = -1) equal to the streaming float32 result bit for bit."""
    n, with_std, flat, sumw, family = CASES_96[name]
    s = stack
    kw = {}
    if flat:
        kw.update(flat=s["flat"], ff_mean=s["ff_mean"])
        if with_std:
            kw.update(flat_std=s["flat_std"], ff_std_mean=s["ff_std_mean"])
    if sumw:
        kw.update(want_sum_w=True)
    fr, sd, t = take(s, n)
    sd = sd if with_std else None
    o64, a32 = both(eng, fr, t, s["icrf"], s["diff"], sd, expect=[family], **kw)
    assert float((o64["val"] > 0).double().mean()) > 0.5                        # a real image, not zeros
    _, g32 = both(eng, fr, t, s["icrf"], s["diff"], sd, expect=["merge_generic"], variant=-1, **kw)
    for k in a32:
        assert torch.equal(a32[k], g32[k]), k
    if "out=f32x4" in family:                              # the pair-store form of the same kernel (variant 32: the store-shape A/B switch)
        _, p32 = both(eng, fr, t, s["icrf"], s["diff"], sd, expect=[family.replace("out=f32x4", "out=f32>")[:-1]], variant=32, **kw)
        assert torch.equal(a32["val"], p32["val"])


def test_f32_streaming_unit_plus_generic_tail(eng):
    """5 x 64 x 3 = 960 elements with N = 7: one unit of 512 in merge_u8_val3 and a generic tail of 448 in one call - the seam where an output
    offset counted in the wrong element size shows."""
    frames, stds, t = orc.synthetic_stack(501, 7, 5, 64, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    fr, sd = [dev(f) for f in frames], [dev(s) for s in stds]
    both(eng, fr, t, icrf, diff, expect=["merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32x4> + merge_generic<f64in=0,std=0,out=f32>"])
    both(eng, fr, t, icrf, diff, expect=["merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32> + merge_generic<f64in=0,std=0,out=f32>"], variant=32)
    both(eng, fr, t, icrf, diff, sd, expect=["merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,out=f32> + merge_generic<f64in=0,std=1,out=f32>"])


@pytest.mark.parametrize("Cc", [1, 2, 4])
@pytest.mark.parametrize("with_std", [False, True])
def test_f32_other_channel_counts(eng, Cc, with_std):
    n, h, w = 7, 40, 52
    frames, stds, t = orc.synthetic_stack(510 + Cc, n, h, w, c=Cc, with_std=with_std)
    icrf = np.stack([np.linspace(0, 1, 256) ** (1.5 + 0.2 * k) for k in range(Cc)], axis=1)
    diff = orc.icrf_derivative(icrf)
    fr = [dev(f) for f in frames]
    sd = [dev(s) for s in stds] if with_std else None
    if Cc == 1:
        family = "merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,C=1,out=f32>" if with_std else "merge_u8_val3<N=7,U=4,PF=1,MAP=3,C=1,out=f32x4>"
    else:
        family = f"merge_u8_loop_std<C={Cc}" if with_std else f"merge_u8_loop<C={Cc}"
    both(eng, fr, t, icrf, diff, sd, expect=[family])
    rng = np.random.default_rng(Cc)
    kw = dict(flat=dev(rng.integers(180, 230, size=(h, w, Cc)).astype(np.uint8)), ff_mean=[0.8, 0.81, 0.79, 0.82][:Cc], want_sum_w=True)
    if with_std:
        kw.update(flat_std=dev(np.full((h, w, Cc), 0.002)), ff_std_mean=[0.002] * Cc)
    _, a32 = both(eng, fr, t, icrf, diff, sd, expect=[f"merge_u8_loop_std<C={Cc},flat=1,sum_w=1,out=f32>" if with_std else f"merge_u8_loop<C={Cc},flat=1,sum_w=1,out=f32>"], **kw)
    _, g32 = both(eng, fr, t, icrf, diff, sd, expect=["merge_generic"], variant=-1, **kw)
    for k in a32:
        assert torch.equal(a32[k], g32[k]), k


@pytest.mark.parametrize("Cc", [3, 1])
def test_f32_float64_frames(eng, Cc):
    n, h, w = 7, 96, 130
    frames, stds, t = orc.synthetic_stack(520 + Cc, n, h, w, c=Cc, with_std=True)
    rng = np.random.default_rng(520)
    f64 = [dev(orc.unit_from_u8(f) + rng.random(f.shape) * 1e-3) for f in frames]
    sd = [dev(s) for s in stds]
    icrf = np.stack([np.linspace(0, 1, 256) ** (1.8 + 0.2 * k) for k in range(Cc)], axis=1)
    diff = orc.icrf_derivative(icrf)
    both(eng, f64, t, icrf, diff, expect=[f"merge_f64_val<C={Cc},flat=0,sum_w=0,out=f32>(N=7)"])
    both(eng, f64, t, icrf, diff, sd, expect=[f"merge_f64_std<C={Cc},flat=0,sum_w=0,out=f32>(N=7)"])
    if Cc == 3:
        # float64 frames that are 8- but not 16-byte aligned: no 16-byte loads, the generic kernel
        odd = []
        for f in f64:
            buf = torch.empty(f.numel() + 1, dtype=torch.float64, device="cuda")
            buf[1:].copy_(f.reshape(-1))
            odd.append(buf[1:].view(h, w, Cc))
        assert odd[0].data_ptr() % 16 == 8
        o64, o32 = both(eng, odd, t, icrf, diff, sd, expect=["merge_generic<f64in=1,std=1,out=f32>"])
        ref64 = eng.merge(f64, t, icrf, diff, sd)
        assert torch.equal(o64["val"], ref64["val"]) and torch.equal(o64["std"], ref64["std"])


def test_f32_row_tiles_at_odd_offsets(eng):
    """n = 3, 11 x 5 x 3 with std: W * C = 15, so tiles at odd rows start at odd element offsets (merge_generic) and at 60-byte offsets of the
    float32 outputs' parent - every tile equals the whole image's rows."""
    n, h, w = 3, 11, 5
    frames, stds, t = orc.synthetic_stack(530, n, h, w, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    fr, sd = [dev(f) for f in frames], [dev(s) for s in stds]
    _, whole = both(eng, fr, t, icrf, diff, sd)
    for r0, r1 in ((1, 4), (3, 11), (0, 1), (10, 11)):
        _, part = both(eng, fr, t, icrf, diff, sd, expect=["merge_generic"], height=h, row0=r0, rows=r1 - r0)
        for k in ("val", "std"):
            assert torch.equal(part[k], whole[k][r0:r1]), (r0, r1, k)


def test_f32_row_tiles_with_median_halo_and_pair_form(eng):
    """Two row tiles with a one-row median halo and dark maps equal the whole image. W * C = 390: the second tile's first element lies
    11 * 390 bytes into the frames - 2- but not 4-byte aligned, so its val-only merge takes the pair-store form of merge_u8_val3, not the
    four-per-lane one."""
    n, h, w = 7, 24, 130
    frames, stds, t = orc.synthetic_stack(531, n, h, w, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    rng = np.random.default_rng(531)
    d = rng.integers(0, 30, size=(h, w, 3)).astype(np.uint8)
    d[0, 0, 0] = d[h - 1, w - 1, 2] = d[10, 5, 1] = d[11, 5, 1] = 255
    darks = [None, None] + [d] * (n - 2)
    mins = [256, 256] + [20] * (n - 2)
    fr, sd, dk = [dev(f) for f in frames], [dev(s) for s in stds], [dev(x) for x in darks]
    for with_std in (False, True):
        s_all = sd if with_std else None
        _, whole = both(eng, fr, t, icrf, diff, s_all, darks=dk, dark_min=mins, median_k=3)
        for r0, r1 in ((0, 11), (11, 24)):
            b0, b1 = max(0, r0 - 1), min(h, r1 + 1)
            expect = [] if with_std else (["merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32x4>"] if r0 == 0 else ["merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32>"])
            _, part = both(eng, [f[b0:b1] for f in fr], t, icrf, diff, None if s_all is None else [s[b0:b1] for s in s_all],
                           darks=[None if x is None else x[b0:b1] for x in dk], dark_min=mins, median_k=3, height=h, row0=r0, rows=r1 - r0, buf_row0=b0,
                           expect=expect)
            for k in part:
                assert torch.equal(part[k], whole[k][r0:r1]), (with_std, r0, k)


@pytest.mark.parametrize("hot_queue", [True, False])
def test_f32_dark_maps(eng, hot_queue):
    """64 x 64 x 3, N = 7, k = 3, with std: hot pixels in the corners, on tile edges and in a run across a wave boundary."""
    n, h, w = 7, 64, 64
    frames, stds, t = orc.synthetic_stack(540, n, h, w, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    rng = np.random.default_rng(540)
    d = rng.integers(0, 10, size=(h, w, 3)).astype(np.uint8)
    d[rng.random(d.shape) < 0.01] = 200
    for y, x, c in ((0, 0, 0), (0, w - 1, 1), (h - 1, 0, 2), (h - 1, w - 1, 0), (31, 0, 1), (32, w - 1, 2)):
        d[y, x, c] = 255
    flat = d.reshape(-1)
    flat[1000:1050] = 255                                  # a run across element 1024: two waves' spans of the scan, several lanes' chunks
    fr, sd, dk = [dev(f) for f in frames], [dev(s) for s in stds], dev(d)
    expect = ["merge_scan_hot + merge_patch_hot<f64in=0,std=1,out=f32>"] if hot_queue else ["merge_fixup_hot<f64in=0,std=1,out=f32>"]
    _, o32 = both(eng, fr, t, icrf, diff, sd, darks=[dk] * n, dark_min=[100] * n, median_k=3, hot_queue=hot_queue, expect=expect)
    # and val-only with a sum of weights through the same pass
    both(eng, fr, t, icrf, diff, darks=[None] + [dk] * (n - 1), dark_min=[256] + [100] * (n - 1), median_k=3, hot_queue=hot_queue, want_sum_w=True)


def test_f32_dark_maps_smallest_workspace_overflow_route(eng):
    from camera_linearity_amd import _native as nat
    n, h, w = 7, 64, 64
    frames, stds, t = orc.synthetic_stack(541, n, h, w, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    rng = np.random.default_rng(541)
    d = (rng.random((h, w, 3)) < 0.02).astype(np.uint8) * 200
    fr, sd, dk = [dev(f) for f in frames], [dev(s) for s in stds], dev(d)
    least = int(nat.lib.hm_merge_hot_workspace_min_bytes(h * w * 3))
    plans = {}
    for dt in (torch.float64, F32):
        p = eng.plan_merge(fr, t, icrf, diff, sd, darks=[dk] * n, dark_min=[100] * n, median_k=3, out_dtype=dt)
        small = torch.zeros(least + 16, dtype=torch.uint8, device="cuda")
        p._keep.append(small)
        p.args.hot_workspace, p.args.hot_workspace_bytes = small.data_ptr(), least
        assert "merge_scan_hot" in p.kernels
        p.launch()
        torch.cuda.synchronize()
        words = small.cpu().numpy()[:16].view(np.uint32)
        assert words[0] >= 1 and words[1] == 1             # something was queued, then the one-entry queue overflowed
        plans[dt] = p
    assert "merge_patch_hot<f64in=0,std=1,out=f32>" in plans[F32].kernels
    for k in ("val", "std"):
        same_bits(plans[F32].outputs[k], plans[torch.float64].outputs[k], k)


@pytest.mark.parametrize("with_std", [False, True])
def test_f32_steady_state(eng, with_std):
    """1024 x 2048 x 3 = 6.3 M elements, N = 7: every wave of the streaming kernels iterates (prefetch ping-pong, both register sets).
    Equality against the float64 call, and the streaming result equal to the generic kernel's."""
    n, h, w = 7, 1024, 2048
    rng = np.random.default_rng(550)
    fr = [torch.as_tensor(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), device="cuda") for _ in range(n)]
    t = list(1e-3 * 2.0 ** np.arange(n))
    icrf, diff = orc.synthetic_icrf()
    sd = [torch.rand((h, w, 3), dtype=torch.float64, device="cuda") * 0.01 for _ in range(n)] if with_std else None
    family = "merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,out=f32>" if with_std else "merge_u8_val3<N=7,U=4,PF=1,MAP=3,out=f32x4>"
    _, a32 = both(eng, fr, t, icrf, diff, sd, expect=[family])
    g32 = eng.merge(fr, t, icrf, diff if with_std else None, sd, variant=-1, out_dtype=F32)
    for k in a32:
        assert torch.equal(a32[k], g32[k]), k
    if not with_std:
        p32 = eng.merge(fr, t, icrf, variant=32, out_dtype=F32)
        assert torch.equal(a32["val"], p32["val"])


def test_f32_range_subnormals_and_overflow(eng, stack):
    """The device's conversion must keep float32 subnormals (no flush to zero) and turn what exceeds float32's maximum into +inf."""
    s = stack
    frames, stds, t = orc.synthetic_stack(580, 7, s["h"], s["w"], with_std=True)     # exposures 1 .. 64 ms
    fr, sd, t = [dev(f) for f in frames], [dev(x) for x in stds], list(t)
    assert min(t) >= 1e-3
    for kw in ({}, dict(variant=-1), dict(variant=32)):
        o64, o32 = both(eng, fr, t, s["icrf"] * 1e-42, s["diff"] * 1e-42, **kw)
        v64, v32 = o64["val"].cpu().numpy(), o32["val"].cpu().numpy()
        assert v64.max() < F32_TINY and (v64 > F32_DENORM_MIN).mean() > 0.9
        sub = v64 > F32_DENORM_MIN
        assert (v32[sub] > 0).all() and (v32[sub] < F32_TINY).all()
    both(eng, fr, t, s["icrf"] * 1e-42, s["diff"] * 1e-42, sd)
    for kw in ({}, dict(variant=-1)):
        o64, o32 = both(eng, fr, [ti * 1e-42 for ti in t], s["icrf"], s["diff"], sd, **kw)
        v64, v32 = o64["val"].cpu().numpy(), o32["val"].cpu().numpy()
        big = v64 > F32_MAX
        assert big.mean() > 0.9 and np.isfinite(v64).all()
        assert (v32[big] == np.inf).all()
    o64, o32 = both(eng, fr, [ti * 1e-42 for ti in t], s["icrf"], s["diff"])
    assert (o32["val"].cpu().numpy()[o64["val"].cpu().numpy() > F32_MAX] == np.inf).all()


def test_f32_plan_graph_replay_equals_eager(eng, stack):
    s = stack
    f7, _, t7 = take(s, 7)
    f15, s15, t15 = take(s, 15)
    p1 = eng.plan_merge(f7, t7, s["icrf"], out_dtype=F32)
    p2 = eng.plan_merge(f15, t15, s["icrf"], s["diff"], s15, flat=s["flat"], flat_std=s["flat_std"], ff_mean=s["ff_mean"],
                        ff_std_mean=s["ff_std_mean"], out_dtype=F32)
    assert "out=f32" in p1.kernels and "out=f32" in p2.kernels
    graph = eng.PlanGraph([p1, p2])
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
            assert p.outputs[k].dtype == F32 and not torch.isnan(p.outputs[k]).any()
            assert torch.equal(p.outputs[k].view(torch.int32), w_[k].view(torch.int32)), k


def test_f32_more_than_32_frames_raises(eng, stack):
    s = stack
    fr = s["fr"] + s["fr"][:1]
    t = s["t"] + [s["t"][-1] * 2]
    with pytest.raises(NotImplementedError):
        eng.merge(fr, t, s["icrf"], out_dtype=F32)
    with pytest.raises(NotImplementedError):
        eng.merge(*take(s, 7)[::2], s["icrf"], variant=-3, out_dtype=F32)
    with pytest.raises(TypeError):
        eng.plan_merge(*take(s, 7)[::2], s["icrf"], out_dtype=torch.float16)


def _features(t):
    return {"illumination": "bf", "magnification": "5x", "exposure": float(t), "subject": "s"}


def test_f32_process_hdr_image_on_the_device(eng, tmp_path):
    """process_HDR_image(out_dtype=torch.float32) with dark and flat lists equals the float64 run cast, on device tensors, without a call
    into the host library; the float32 measurand computes (upcast) and saves."""
    from camera_linearity_amd import _native as nat
    from camera_linearity_amd import settings as gs
    from camera_linearity_amd import tiff_io
    from camera_linearity_amd.exposure_series import ExposureSeries
    from camera_linearity_amd.image_set import ImageSet
    n, h, w = 5, 48, 40
    frames, stds, t = orc.synthetic_stack(560, n, h, w, with_std=True)
    icrf, diff = orc.synthetic_icrf()
    rng = np.random.default_rng(560)
    dark = rng.integers(0, 4, size=(h, w, 3)).astype(np.uint8)
    dark[rng.random(dark.shape) < 0.01] = 200
    flat = rng.integers(180, 230, size=(h, w, 3)).astype(np.uint8)
    old = (gs.DARK_THRESHOLD, gs.FF_MID_PERCENTAGE, gs.MEDIAN_FILTER_KERNEL_SIZE)
    gs.configure(DARK_THRESHOLD=0.05, FF_MID_PERCENTAGE=0.2, MEDIAN_FILTER_KERNEL_SIZE=3)
    try:
        host_calls = sum(nat.host_lib().calls.values())

        def run(out_dtype):
            sets = [ImageSet(value=f, std=s_.copy(), features=_features(ti), use_cupy=True) for f, s_, ti in zip(frames, stds, t)]
            darks = [ImageSet(value=dark, features=dict(_features(ti), subject="dark"), use_cupy=True) for ti in t[1:]]
            fl = ImageSet(value=flat, std=np.full(flat.shape, 0.002), features=dict(_features(0.01), subject="flat"), use_cupy=True)
            series = ExposureSeries(input_image_sets=sets)
            series.process_HDR_image(icrf, diff, dark_list=darks, flat_list=[fl], out_dtype=out_dtype)
            return series.merged_image_set
        hdr64, hdr32 = run(None), run(F32)
        m64, m32 = hdr64.measurand, hdr32.measurand
        assert m32.val.is_cuda and m32.val.dtype == F32 and m32.std.dtype == F32 and m64.val.dtype == torch.float64
        same_bits(m32.val, m64.val, "val")
        same_bits(m32.std, m64.std, "std")
        doubled, up = m32 * 2.0, type(m32)(m32.val.double(), m32.std.double()) * 2.0
        assert doubled.val.dtype == torch.float64 and torch.equal(doubled.val, up.val) and torch.equal(doubled.std, up.std)
        assert sum(nat.host_lib().calls.values()) == host_calls             # the device run never entered the host library
        hdr32.path = tmp_path / "s bf 5x.tif"
        hdr32.save_32bit(is_HDR=True)
        back = tiff_io.imread(tmp_path / "32bit" / "s bf 5x HDR.tif", tiff_io.IMREAD_UNCHANGED)
        assert back.dtype == np.float32 and np.array_equal(back.view(np.int32), m32.val.cpu().numpy().view(np.int32))
        hdr32.save_64bit(tmp_path / "w" / "y.tif", device_encode=True)
        assert np.array_equal(tiff_io.imread(tmp_path / "w" / "y.tif", tiff_io.IMREAD_UNCHANGED), m32.val.double().cpu().numpy())
    finally:
        gs.configure(DARK_THRESHOLD=old[0], FF_MID_PERCENTAGE=old[1], MEDIAN_FILTER_KERNEL_SIZE=old[2])


@pytest.mark.parametrize("with_std", [False, True])
def test_f32_merge_pipeline(eng, with_std):
    from camera_linearity_amd.pipeline import MergePipeline
    n, h, w = 7, 40, 52
    icrf, diff = orc.synthetic_icrf()
    stacks, sds = [], []
    for k in range(3):
        frames, stds, t = orc.synthetic_stack(570 + k, n, h, w, with_std=True)
        stacks.append(frames)
        sds.append(stds)
    got = {}
    for dt in (torch.float64, F32):
        pipe = MergePipeline(n, h, w, t, icrf, diff if with_std else None, with_std=with_std, out_dtype=dt)
        assert pipe.slots[0].h_val.dtype == dt and pipe.slots[0].plan.outputs["val"].dtype == dt
        got[dt] = pipe.merge_many(stacks, sds if with_std else None)
    for (v64, s64), (v32, s32) in zip(got[torch.float64], got[F32]):
        same_bits(torch.from_numpy(v32), torch.from_numpy(v64), "val")
        if with_std:
            same_bits(torch.from_numpy(s32), torch.from_numpy(s64), "std")
