"""The fused merge with its stds from the per-DN STD table (engine.plan_merge(std_table=...), hm_merge_std_table) on the MI355X.

Exact criterion, no tolerance: the table merge equals the std-stream merge of the same plan inputs fed stds[i] = linearize(frame_i, None,
std_table)[0] made on the device, compared as integer bit patterns - and both equal the generic kernel (variant = -1). Every case asserts
through plan.kernels which kernel family ran. Tables are random per (DN, c) - not monotone - with exact zeros and one subnormal."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import hdr_oracle as orc  # noqa: E402

F32 = torch.float32


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from camera_linearity_amd import engine
    return engine


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(out32, out64, what=""):
    """The rule of tests/test_gpu_merge_f32.py: float32 output == NumPy's conversion of the float64 output."""
    a, b = out64.cpu().numpy(), out32.cpu().numpy()
    assert a.dtype == np.float64 and b.dtype == np.float32 and a.shape == b.shape, (what, a.dtype, b.dtype)
    with np.errstate(over="ignore", under="ignore"):
        want = a.astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(b)), what
    bad = want.view(np.int32)[~nan] != b.view(np.int32)[~nan]
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8])


def make_table(seed, c):
    rng = np.random.default_rng(seed)
    tab = rng.random((256, c)) * 0.02
    tab[rng.random((256, c)) < 0.05] = 0.0
    tab[17, 0] = 5e-324
    return tab


def device_stds(eng, fr, table):
    return [eng.linearize(f, None, table)[0] for f in fr]


def table_vs_stream(eng, fr, t, icrf, diff, table, expect=(), sd=None, **kw):
    """Table plan against the std-stream plan of the same inputs; `expect`: substrings the table plan's kernels must hold. -> table outputs."""
    sd = device_stds(eng, fr, table) if sd is None else sd
    ps = eng.plan_merge(fr, t, icrf, diff, sd, **kw)
    pt = eng.plan_merge(fr, t, icrf, diff, std_table=table, **kw)
    names = pt.kernels
    for e in expect:
        assert e in names, (e, names)
    for part in names.split(" + "):
        assert "std=lut" in part or part == "merge_scan_hot", names
    assert "lut" not in ps.kernels
    for v in pt.outputs.values():
        v.fill_(float("nan"))
    ps.launch()
    pt.launch()
    torch.cuda.synchronize()
    assert ps.outputs.keys() == pt.outputs.keys() and "std" in pt.outputs
    for k in ps.outputs:
        assert torch.equal(bits(pt.outputs[k]), bits(ps.outputs[k])), (k, names)
    assert ps.algorithmic_bytes - pt.algorithmic_bytes == 8 * len(fr) * pt.outputs["val"].numel()
    return pt.outputs


@pytest.fixture(scope="module")
def stack(eng):
    """96 x 130 x 3, 32 frames, flat field, tables and the device-linearized stds - made once, never written."""
    h, w = 96, 130
    frames, _, t = orc.synthetic_stack(600, 32, h, w)
    icrf, diff = orc.synthetic_icrf()
    rng = np.random.default_rng(600)
    flat = rng.integers(180, 230, size=(h, w, 3)).astype(np.uint8)
    table = make_table(600, 3)
    fr = [dev(f) for f in frames]
    return dict(fr=fr, sd=device_stds(eng, fr, table), t=list(t), icrf=icrf, diff=diff, table=table, flat=dev(flat),
                flat_std=dev(np.full((h, w, 3), 0.002)), ff_mean=[0.8, 0.81, 0.79], ff_std_mean=[0.002] * 3, h=h, w=w)


def take(stack, n):
    lo = max(0, min(16 - n // 2, 32 - n))
    return stack["fr"][lo:lo + n], stack["sd"][lo:lo + n], stack["t"][lo:lo + n]


CASES_96 = {
    # name: (n, flat, sum_w, kernel family of the table plan)
    "n7": (7, False, False, "merge_u8_fast_std<N=7,U=1,flat=0,sum_w=0,std=lut>"),
    "n7_flat": (7, True, False, "merge_u8_fast_std<N=7,U=1,flat=1,sum_w=0,std=lut>"),
    "n7_sumw": (7, False, True, "merge_u8_loop_std<C=3,flat=0,sum_w=1,std=lut>(N=7)"),           # sum_w with a table streams at run-time N
    "n7_flat_sumw": (7, True, True, "merge_u8_loop_std<C=3,flat=1,sum_w=1,std=lut>(N=7)"),
    "n15": (15, False, False, "merge_u8_fast_std<N=15,U=1,flat=0,sum_w=0,std=lut>"),
    "n15_flat": (15, True, False, "merge_u8_fast_std<N=15,U=1,flat=1,sum_w=0,std=lut>"),
    "n15_flat_sumw": (15, True, True, "merge_u8_loop_std<C=3,flat=1,sum_w=1,std=lut>(N=15)"),
    "n20": (20, False, False, "merge_u8_loop_std<C=3,flat=0,sum_w=0,std=lut>(N=20)"),
    "n21": (21, False, False, "merge_u8_loop_std<C=3,flat=0,sum_w=0,std=lut>(N=21)"),
    "n32_flat": (32, True, False, "merge_u8_loop_std<C=3,flat=1,sum_w=0,std=lut>(N=32)"),
}


@pytest.mark.parametrize("name", list(CASES_96))
def test_table_equals_stream_96x130(eng, stack, name):
    """Every streaming family at 37 440 elements (whole groups + a generic tail, more than one workgroup); float64 and float32 outputs;
    the generic kernel gives the same bits."""
    n, flat, sumw, family = CASES_96[name]
    s = stack
    kw = {}
    if flat:
        kw.update(flat=s["flat"], ff_mean=s["ff_mean"], flat_std=s["flat_std"], ff_std_mean=s["ff_std_mean"])
    if sumw:
        kw.update(want_sum_w=True)
    fr, sd, t = take(s, n)
    out = table_vs_stream(eng, fr, t, s["icrf"], s["diff"], s["table"], expect=[family, "merge_generic"], sd=sd, **kw)
    assert float((out["val"] > 0).double().mean()) > 0.5 and float((out["std"] > 0).double().mean()) > 0.5
    gen = table_vs_stream(eng, fr, t, s["icrf"], s["diff"], s["table"], expect=["merge_generic<f64in=0,std=1,std=lut>"], sd=sd, variant=-1, **kw)
    assert "merge_u8" not in eng.plan_merge(fr, t, s["icrf"], s["diff"], std_table=s["table"], variant=-1, **kw).kernels
    for k in out:
        assert torch.equal(bits(out[k]), bits(gen[k])), k
    o32 = table_vs_stream(eng, fr, t, s["icrf"], s["diff"], s["table"], expect=["out=f32"], sd=sd, out_dtype=F32, **kw)
    for k in ("val", "std"):
        same_bits(o32[k], out[k], k)


@pytest.mark.parametrize("Cc", [1, 2, 4])
def test_table_other_channel_counts(eng, Cc):
    n, h, w = 7, 40, 52
    frames, _, t = orc.synthetic_stack(610 + Cc, n, h, w, c=Cc)
    icrf = np.stack([np.linspace(0, 1, 256) ** (1.5 + 0.2 * k) for k in range(Cc)], axis=1)
    diff = orc.icrf_derivative(icrf)
    table = make_table(610 + Cc, Cc)
    fr = [dev(f) for f in frames]
    rng = np.random.default_rng(Cc)
    kw = dict(flat=dev(rng.integers(180, 230, size=(h, w, Cc)).astype(np.uint8)), ff_mean=[0.8, 0.81, 0.79, 0.82][:Cc], want_sum_w=True,
              flat_std=dev(np.full((h, w, Cc), 0.002)), ff_std_mean=[0.002] * Cc)
    a = table_vs_stream(eng, fr, list(t), icrf, diff, table, expect=[f"merge_u8_loop_std<C={Cc},flat=0,sum_w=0,std=lut>(N=7)"])
    b = table_vs_stream(eng, fr, list(t), icrf, diff, table, expect=[f"merge_u8_loop_std<C={Cc},flat=1,sum_w=1,std=lut>(N=7)"], **kw)
    for out, k2 in ((a, {}), (b, kw)):
        gen = table_vs_stream(eng, fr, list(t), icrf, diff, table, expect=["merge_generic"], variant=-1, **k2)
        for k in out:
            assert torch.equal(bits(out[k]), bits(gen[k])), k


def test_table_float64_frames(eng):
    """float64 frames stream through merge_generic with a table: .5 ties (round half to even) and values above 1.0 that wrap the index."""
    n, h, w = 5, 40, 52
    frames, _, t = orc.synthetic_stack(620, n, h, w)
    rng = np.random.default_rng(620)
    f64 = []
    for f in frames:
        v = (f.astype(np.float64) + rng.choice([0.0, 0.5, 0.25, -0.25], size=f.shape)) / 255.0
        v[rng.random(f.shape) < 0.05] += 1.0
        f64.append(dev(v))
    icrf, diff = orc.synthetic_icrf()
    table = make_table(620, 3)
    out = table_vs_stream(eng, f64, list(t), icrf, diff, table, expect=["merge_generic<f64in=1,std=1,std=lut>"])
    o32 = table_vs_stream(eng, f64, list(t), icrf, diff, table, expect=["merge_generic<f64in=1,std=1,std=lut,out=f32>"], out_dtype=F32)
    same_bits(o32["std"], out["std"])
    d = rng.integers(0, 10, size=(h, w, 3)).astype(np.uint8)
    d[rng.random(d.shape) < 0.02] = 200
    for hq in (True, False):
        table_vs_stream(eng, f64, list(t), icrf, diff, table, darks=[dev(d)] * n, dark_min=[100] * n, median_k=3, hot_queue=hq,
                        expect=["merge_patch_hot<f64in=1,std=1,std=lut>" if hq else "merge_fixup_hot<f64in=1,std=1,std=lut>"])


def test_table_row_tiles_with_median_halo(eng):
    """Row tiles at odd offsets (W * C = 15: merge_generic) and two tiles with a one-row median halo and dark maps equal the whole image."""
    icrf, diff = orc.synthetic_icrf()
    table = make_table(630, 3)
    n, h, w = 3, 11, 5
    frames, _, t = orc.synthetic_stack(630, n, h, w)
    fr = [dev(f) for f in frames]
    whole = table_vs_stream(eng, fr, list(t), icrf, diff, table)
    for r0, r1 in ((1, 4), (3, 11), (10, 11)):
        part = table_vs_stream(eng, fr, list(t), icrf, diff, table, expect=["merge_generic"], height=h, row0=r0, rows=r1 - r0)
        for k in ("val", "std"):
            assert torch.equal(bits(part[k]), bits(whole[k][r0:r1])), (r0, r1, k)
    n, h, w = 7, 24, 130
    frames, _, t = orc.synthetic_stack(631, n, h, w)
    rng = np.random.default_rng(631)
    d = rng.integers(0, 30, size=(h, w, 3)).astype(np.uint8)
    d[0, 0, 0] = d[h - 1, w - 1, 2] = d[10, 5, 1] = d[11, 5, 1] = 255
    fr, dk = [dev(f) for f in frames], [None, None] + [dev(d)] * (n - 2)
    mins = [256, 256] + [20] * (n - 2)
    whole = table_vs_stream(eng, fr, list(t), icrf, diff, table, darks=dk, dark_min=mins, median_k=3)
    for r0, r1 in ((0, 11), (11, 24)):
        b0, b1 = max(0, r0 - 1), min(h, r1 + 1)
        part = table_vs_stream(eng, [f[b0:b1] for f in fr], list(t), icrf, diff, table, darks=[None if x is None else x[b0:b1] for x in dk],
                               dark_min=mins, median_k=3, height=h, row0=r0, rows=r1 - r0, buf_row0=b0)
        for k in part:
            assert torch.equal(bits(part[k]), bits(whole[k][r0:r1])), (r0, k)


def _dark_case(seed, density=0.01):
    n, h, w = 7, 64, 64
    frames, _, t = orc.synthetic_stack(seed, n, h, w)
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, size=f.shape).astype(np.uint8) for f in frames]       # rough neighbourhoods: the two median rules differ
    d = rng.integers(0, 10, size=(h, w, 3)).astype(np.uint8)
    d[rng.random(d.shape) < density] = 200
    for y, x, c in ((0, 0, 0), (0, w - 1, 1), (h - 1, 0, 2), (h - 1, w - 1, 0), (31, 0, 1), (32, w - 1, 2)):
        d[y, x, c] = 255
    d.reshape(-1)[1000:1050] = 255
    return n, h, w, frames, list(t), d


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("hot_queue", [True, False])
def test_table_dark_maps(eng, hot_queue, k):
    n, h, w, frames, t, d = _dark_case(640)
    icrf, diff = orc.synthetic_icrf()
    table = make_table(640, 3)
    hot = d >= 100                                          # from the inputs alone: the two median rules differ on a hot element
    mapped = np.stack([table[frames[0][..., c], c] for c in range(3)], axis=-1)
    med_dn = orc.median_filter_reflect(frames[0].astype(np.float64), k).astype(np.uint8)
    other = np.stack([table[med_dn[..., c], c] for c in range(3)], axis=-1)
    assert ((orc.median_filter_reflect(mapped, k) != other) & hot).any()
    fr, dk = [dev(f) for f in frames], dev(d)
    expect = ["merge_scan_hot + merge_patch_hot<f64in=0,std=1,std=lut>"] if hot_queue else ["merge_fixup_hot<f64in=0,std=1,std=lut>"]
    out = table_vs_stream(eng, fr, t, icrf, diff, table, darks=[dk] * n, dark_min=[100] * n, median_k=k, hot_queue=hot_queue, expect=expect)
    o32 = table_vs_stream(eng, fr, t, icrf, diff, table, darks=[None] + [dk] * (n - 1), dark_min=[256] + [100] * (n - 1), median_k=k,
                          hot_queue=hot_queue, want_sum_w=True, out_dtype=F32)
    assert o32["std"].dtype == F32 and not torch.isnan(out["std"]).any()


def test_table_dark_maps_smallest_workspace(eng):
    from camera_linearity_amd import _native as nat
    n, h, w, frames, t, d = _dark_case(641, density=0.02)
    icrf, diff = orc.synthetic_icrf()
    table = make_table(641, 3)
    fr, dk = [dev(f) for f in frames], dev(d)
    want = eng.merge(fr, t, icrf, diff, device_stds(eng, fr, table), darks=[dk] * n, dark_min=[100] * n, median_k=3)
    least = int(nat.lib.hm_merge_hot_workspace_min_bytes(h * w * 3))
    p = eng.plan_merge(fr, t, icrf, diff, std_table=table, darks=[dk] * n, dark_min=[100] * n, median_k=3)
    small = torch.zeros(least + 16, dtype=torch.uint8, device="cuda")
    p._keep.append(small)
    p.args.hot_workspace, p.args.hot_workspace_bytes = small.data_ptr(), least
    assert "merge_scan_hot + merge_patch_hot<f64in=0,std=1,std=lut>" in p.kernels
    p.launch()
    torch.cuda.synchronize()
    words = small.cpu().numpy()[:16].view(np.uint32)
    assert words[0] >= 1 and words[1] == 1                 # something was queued, then the one-entry queue overflowed
    for k in ("val", "std"):
        assert torch.equal(bits(p.outputs[k]), bits(want[k])), k


def test_table_second_launch_and_graph_replay(eng, stack):
    s = stack
    f7, _, t7 = take(s, 7)
    f21, _, t21 = take(s, 21)
    p1 = eng.plan_merge(f7, t7, s["icrf"], s["diff"], std_table=s["table"])
    p2 = eng.plan_merge(f21, t21, s["icrf"], s["diff"], std_table=s["table"], flat=s["flat"], flat_std=s["flat_std"], ff_mean=s["ff_mean"],
                        ff_std_mean=s["ff_std_mean"], out_dtype=F32)
    for p in (p1, p2):
        p.launch()
    torch.cuda.synchronize()
    want = [{k: v.clone() for k, v in p.outputs.items()} for p in (p1, p2)]

    def check(what):
        torch.cuda.synchronize()
        for p, w_ in zip((p1, p2), want):
            for k in w_:
                assert torch.equal(bits(p.outputs[k]), bits(w_[k])), (what, k)
            for v in p.outputs.values():
                v.fill_(float("nan"))
    check("first")
    for p in (p1, p2):
        p.launch()
    check("second launch")
    graph = eng.PlanGraph([p1, p2])
    check("graph warm-up")
    graph.replay()
    check("replay")


def test_table_more_than_32_frames_raises(eng, stack):
    s = stack
    with pytest.raises(NotImplementedError):
        eng.merge(s["fr"] + s["fr"][:1], s["t"] + [s["t"][-1] * 2], s["icrf"], s["diff"], std_table=s["table"])
    with pytest.raises(NotImplementedError):
        eng.merge(*take(s, 7)[::2], s["icrf"], s["diff"], std_table=s["table"], variant=-3)
    with pytest.raises(ValueError):
        eng.merge(*take(s, 7)[::2], s["icrf"], s["diff"], take(s, 7)[1], std_table=s["table"])


def test_table_merge_pipeline(eng):
    from camera_linearity_amd.pipeline import MergePipeline
    n, h, w = 7, 40, 52
    icrf, diff = orc.synthetic_icrf()
    table = make_table(650, 3)
    stacks = []
    for k in range(3):
        frames, _, t = orc.synthetic_stack(650 + k, n, h, w)
        stacks.append(frames)
    pipe = MergePipeline(n, h, w, t, icrf, diff, std_table=table)
    for slot in pipe.slots:                                 # a std output, no std buffers on either side of the bus
        assert slot.h_stds is None and slot.d_stds is None and slot.h_std is not None and "std=lut" in slot.plan.kernels
    assert pipe.input_views(0)[1] is None
    got = pipe.merge_many(stacks)
    for frames, (val, std) in zip(stacks, got):
        want = eng.merge([dev(f) for f in frames], list(t), icrf, diff, std_table=table)
        assert np.array_equal(val.view(np.int64), want["val"].cpu().numpy().view(np.int64))
        assert np.array_equal(std.view(np.int64), want["std"].cpu().numpy().view(np.int64))
    with pytest.raises(ValueError):
        MergePipeline(n, h, w, t, icrf, diff, with_std=True, std_table=table)


def _features(t):
    return {"illumination": "bf", "magnification": "5x", "exposure": float(t), "subject": "s"}


def test_table_process_hdr_image_on_the_device(eng):
    from camera_linearity_amd import _native as nat
    from camera_linearity_amd.exposure_series import ExposureSeries
    from camera_linearity_amd.image_set import ImageSet
    n, h, w = 5, 48, 40
    frames, _, t = orc.synthetic_stack(660, n, h, w)
    icrf, diff = orc.synthetic_icrf()
    rng = np.random.default_rng(660)
    table = make_table(660, 3)
    dark = rng.integers(0, 4, size=(h, w, 3)).astype(np.uint8)
    dark[rng.random(dark.shape) < 0.01] = 200
    flat = rng.integers(180, 230, size=(h, w, 3)).astype(np.uint8)

    def run(materialise):
        sets = [ImageSet(value=f, features=_features(ti), use_cupy=True) for f, ti in zip(frames, t)]
        darks = [ImageSet(value=dark, features=dict(_features(ti), subject="dark"), use_cupy=True) for ti in t[1:]]
        fl = ImageSet(value=flat, std=np.full(flat.shape, 0.002), features=dict(_features(0.01), subject="flat"), use_cupy=True)
        series = ExposureSeries(input_image_sets=sets)
        if materialise:
            for im in sets:
                im.load_std_image(table)
            series.process_HDR_image(icrf, diff, dark_list=darks, flat_list=[fl])
        else:
            series.process_HDR_image(icrf, diff, dark_list=darks, flat_list=[fl], STD_data=table)
            assert all(im.measurand.std is None for im in sets)
        return series.merged_image_set.measurand
    want = run(True)
    calls = dict(nat.hip_lib.calls)
    got = run(False)
    assert nat.hip_lib.calls["hm_merge_std_table"] == calls.get("hm_merge_std_table", 0) + 1
    assert nat.hip_lib.calls["hm_linearize_u8"] == calls.get("hm_linearize_u8", 0)
    assert got.val.is_cuda and torch.equal(bits(got.val), bits(want.val)) and torch.equal(bits(got.std), bits(want.std))
