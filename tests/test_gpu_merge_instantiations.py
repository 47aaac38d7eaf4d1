"""Every templated instantiation of the fused merge launches and matches merge_generic bit for bit (MI355X).

The compile-time-N kernels (merge_u8_val3, merge_u8_fast, merge_u8_fast_std and its per-DN-table form) are instantiated per frame count
in several translation units; losing or mislinking one frame count would go unnoticed by tests that launch a few of them. Here every
N in 1..20 is launched in every configuration that has a kernel of its own, on the smallest shape that holds a whole group of every unit
size in use (128, 256, 384, 512 elements) plus a tail: 12 x 44 x 3 = 12 x 132 x 1 = 1 584 elements = 3 x 512 + 48. The criterion is
exact: the outputs equal those of the same call with variant = -1 (merge_generic alone), and plan.kernels names the templated kernel."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import hdr_oracle as orc  # noqa: E402

H, W3, W1 = 12, 44, 132
F32 = torch.float32


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from camera_linearity_amd import engine
    return engine


@pytest.fixture(scope="module")
def data():
    """20 frames + stds, flat field, ICRF and a std table for C = 3 and C = 1; a case takes the first n frames. Made once, never written to."""
    out = {}
    icrf3, diff3 = orc.synthetic_icrf()
    for c, w in ((3, W3), (1, W1)):
        rng = np.random.default_rng(40 + c)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")                    # noqa: E731
        out[c] = dict(
            frames=[up(rng.integers(0, 256, (H, w, c), dtype=np.uint8)) for _ in range(20)],
            stds=[up(0.004 * (1 + rng.random((H, w, c)))) for _ in range(20)],
            t=[1e-3 * 1.3 ** i for i in range(20)],
            icrf=icrf3[:, :c].copy(), diff=diff3[:, :c].copy(),
            table=rng.random((256, c)) * 0.02,
            flat=up(rng.integers(150, 250, (H, w, c), dtype=np.uint8)), flat_std=up(np.full((H, w, c), 0.002)),
            ff_mean=[0.8, 0.81, 0.79][:c], ff_std_mean=[0.002] * c)
    return out


def run(eng, d, n, expect, std=None, flat=False, sum_w=False, out_dtype=torch.float64, variant=0):
    """One configuration on the first n frames against its variant = -1 twin; `expect`: regex the streaming kernel's name must match."""
    kw = dict(out_dtype=out_dtype)
    if std == "frames":
        kw["stds"] = d["stds"][:n]
    elif std == "table":
        kw["std_table"] = d["table"]
    if flat:
        kw.update(flat=d["flat"], ff_mean=d["ff_mean"])
        if std:
            kw.update(flat_std=d["flat_std"], ff_std_mean=d["ff_std_mean"])
    if sum_w:
        kw["want_sum_w"] = True
    plans = [eng.plan_merge(d["frames"][:n], d["t"][:n], d["icrf"], d["diff"] if std else None, variant=v, **kw) for v in (variant, -1)]
    fast, ref = plans
    body, _, tail = fast.kernels.partition(" + ")
    assert re.fullmatch(expect, body), (expect, fast.kernels)
    assert tail.startswith("merge_generic<") and ref.kernels.startswith("merge_generic<") and " + " not in ref.kernels, (fast.kernels, ref.kernels)
    for p in plans:
        for v in p.outputs.values():
            v.fill_(float("nan"))
        p.launch()
    torch.cuda.synchronize()
    assert fast.outputs.keys() == ref.outputs.keys()
    for k in ref.outputs:
        assert not torch.isnan(ref.outputs[k]).any(), k
        assert torch.equal(fast.outputs[k], ref.outputs[k]), (k, fast.kernels)


@pytest.mark.parametrize("n", range(1, 21))
def test_colour_instantiations_match_generic(eng, data, n):
    d = data[3]
    run(eng, d, n, rf"merge_u8_val3<N={n},U=\d,PF=\d,MAP=\d>")
    run(eng, d, n, rf"merge_u8_fast_std<N={n},U=1,flat=0,sum_w=0>", std="frames")
    if n <= 16:
        run(eng, d, n, rf"merge_u8_fast_std<N={n},U=1,flat=0,sum_w=0,std=lut>", std="table")
    # (a uint8 flat field, val-only: merge_u8_val3's flat-field instantiation up to 16 frames, merge_u8_fast's above)
    run(eng, d, n, rf"merge_u8_val3<N={n},U=\d,PF=\d,MAP=\d,flat=1>" if n <= 16 else rf"merge_u8_fast<N={n},U=2,flat=1,sum_w=0>", flat=True)
    run(eng, d, n, rf"merge_u8_fast_std<N={n},U=1,flat=1,sum_w=1>", std="frames", flat=True, sum_w=True)


@pytest.mark.parametrize("n", range(1, 17))
def test_monochrome_instantiations_match_generic(eng, data, n):
    d = data[1]
    run(eng, d, n, rf"merge_u8_val3<N={n},U=\d,PF=\d,MAP=\d,C=1>")
    run(eng, d, n, rf"merge_u8_val3<N={n},U=\d,PF=\d,MAP=\d,flat=1,C=1>", flat=True)
    run(eng, d, n, rf"merge_u8_fast_std<N={n},U=1,flat=0,sum_w=0,C=1>", std="frames")
    run(eng, d, n, rf"merge_u8_fast_std<N={n},U=1,flat=1,sum_w=0,C=1>", std="frames", flat=True)


@pytest.mark.parametrize("n", [7, 15])
def test_float32_instantiations_match_generic(eng, data, n):
    d, m = data[3], data[1]
    quad = "out=f32x4" if n == 7 else "out=f32"           # N = 7 runs <U=4,PF=1>: whole 256-element spans; N = 15 runs the in-place refill
    run(eng, d, n, rf"merge_u8_val3<N={n},U=\d,PF=\d,MAP=\d,{quad}>", out_dtype=F32)
    run(eng, d, n, rf"merge_u8_val3<N={n},U=\d,PF=\d,MAP=\d,out=f32>", out_dtype=F32, variant=32)           # the pair map forced
    run(eng, d, n, rf"merge_u8_val3<N={n},U=\d,PF=\d,MAP=\d,flat=1,out=f32(x4)?>", out_dtype=F32, flat=True)
    run(eng, d, n, rf"merge_u8_fast<N={n},U=2,flat=0,sum_w=1,out=f32>", out_dtype=F32, sum_w=True)
    run(eng, d, n, rf"merge_u8_fast_std<N={n},U=1,flat=0,sum_w=0,out=f32>", out_dtype=F32, std="frames")
    run(eng, d, n, rf"merge_u8_fast_std<N={n},U=1,flat=1,sum_w=1,out=f32>", out_dtype=F32, std="frames", flat=True, sum_w=True)
    run(eng, m, n, rf"merge_u8_val3<N={n},U=\d,PF=\d,MAP=\d,C=1,out=f32(x4)?>", out_dtype=F32)
    run(eng, m, n, rf"merge_u8_fast_std<N={n},U=1,flat=0,sum_w=0,C=1,out=f32>", out_dtype=F32, std="frames")
