"""The fused merge on uint16 DN frames (hm_merge_u16, hm_linearize_u16) on the GPU: the checks of tests/test_merge_u16_host.py - embedding
of an 8-bit stack bit for bit against the 8-bit kernels, the NumPy restatement, masking - for every forced variant that applies (-1 one
element per thread, 1 tables in LDS, 2 tables in global memory, 3 tables split between the two) and the default, with plan.kernels
asserting which kernel and which table placement ran; variants against each other; float32 outputs; hipGraph replay; TIFF round trip.

Shapes are the smallest that cross every boundary of the kernels: (13, 37, 3) several wave groups of 128 elements plus a tail that goes to
the generic kernel, (8, 64, 4) whole groups only, (3, 43, 1) and (7, 33, 2); a row tile of a 16-row image at an even input offset
(streams) and at an odd one (generic); N = 1, 2, 7, 9 (one chunk of the loop plus one frame) and 32; depths 9, 10, 12, 16 and, for
C = 3 and C = 4, the largest depth whose tables the fit rule puts in LDS and the first it does not, with and without stds."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_merge_u16_host as h16  # noqa: E402
from test_merge_u16_host import DEPTHS, F32, FIT, SHAPES, T, assert_same_bits, exposures, full_range_frames, make_stds, tables_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from camera_linearity_amd import engine
    assert torch.cuda.is_available()
    return engine


fits = h16.fits_lds


def variants_for(c, b, with_std):
    """The default and every forced variant that is legal: -1 one element per thread, 1 tables in LDS, 2 in global memory, 3 split."""
    return (-1, 2, 0) + ((1,) if fits(c, b, with_std) else ()) + ((3,) if h16.mixed_placement(c, b, with_std) else ())


def expect_kernels(c, b, with_std, pairs_ok=True, streams=True):
    """plan.kernels of a call with E output elements under variant v: the streaming kernel on whole groups of 128 with its tables where
    the variant / the fit rule puts them, the generic kernel on the tail - or on everything."""
    def expect(v, names, E):
        parts = names.split(" + ")
        assert all(f"bits={b}," in p for p in parts), names
        if v == -1 or not pairs_ok or not streams or E < 128:
            assert len(parts) == 1 and parts[0].startswith("merge_u16_generic<"), (v, names)
            return
        tab = h16.placement(c, b, with_std, v)
        assert parts[0].startswith(f"merge_u16_stream<tab={tab},bits={b},C={c},std={int(with_std)},"), (v, names)
        assert len(parts) == (2 if E % 128 else 1) and all(p.startswith("merge_u16_generic<") for p in parts[1:]), (v, names)
    return expect


# ---------------------------------------------------------------------------------------------- 1. embedding
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("b", DEPTHS)
@pytest.mark.parametrize("with_std", [False, True], ids=["val", "std"])
def test_embedding(eng, shape, b, with_std):
    c = shape[2]
    h16.check_embedding(eng, DEV, shape, 9 if with_std else 7, b, with_std, variants_for(c, b, with_std), expect=expect_kernels(c, b, with_std))


@pytest.mark.parametrize("c,with_std", [(3, False), (3, True), (4, False), (4, True)])
def test_embedding_at_the_fit_boundary(eng, c, with_std):
    """The largest depth whose tables all live in LDS (C = 4: exactly 160 KiB) and the first that keeps only a part of them there."""
    b = FIT[(c, with_std)]
    shape = (13, 37, 3) if c == 3 else (8, 64, 4)
    for depth in (b, b + 1):
        names = h16.check_embedding(eng, DEV, shape, 7, depth, with_std, variants_for(c, depth, with_std), expect=expect_kernels(c, depth, with_std))
        assert ("tab=lds" in names[0]) == (depth == b) and (1 in names) == (depth == b) and 3 in names and "tab=mixed-" in names[3]
    with pytest.raises(NotImplementedError):                 # variant 1 where the tables do not fit: refused when the plan is built
        h16.check_embedding(eng, DEV, shape, 7, b + 1, with_std, (1,))


@pytest.mark.parametrize("n", [1, 2, 7, 9, 32])
def test_embedding_frame_counts(eng, n):
    for b, with_std in ((12, False), (10, True), (16, True)):
        h16.check_embedding(eng, DEV, (13, 37, 3), n, b, with_std, variants_for(3, b, with_std), expect=expect_kernels(3, b, with_std), want_sum_w=True)
    # the sum-of-weights-only call: one element per thread whatever the variant
    h16.check_embedding(eng, DEV, (13, 37, 3), n, 12, False, (0, 1, 2, -1), expect=expect_kernels(3, 12, False, streams=False), want_val=False, want_sum_w=True)


@pytest.mark.parametrize("with_std", [False, True], ids=["val", "std"])
@pytest.mark.parametrize("out_dtype", [torch.float64, F32], ids=["f64", "f32"])
def test_embedding_flat_field_and_outputs(eng, with_std, out_dtype):
    rng = np.random.default_rng(21)
    for shape, b in (((13, 37, 3), 12 if not with_std else 10), ((8, 64, 4), 16), ((3, 43, 1), 9)):
        h, w, c = shape
        names = h16.check_embedding(eng, DEV, shape, 7, b, with_std, variants_for(c, b, with_std), expect=expect_kernels(c, b, with_std),
                                    want_sum_w=True, out_dtype=out_dtype, **h16.flat_kw(rng, h, w, c, with_std))
        assert all(("out=f32" in v) == (out_dtype == F32) and "flat=1,sum_w=1" in v for v in names.values())


@pytest.mark.parametrize("with_std", [False, True], ids=["val", "std"])
def test_embedding_row_tiles(eng, with_std):
    """Rows [row0, row0 + 6) of a 16-row image from buffers that start at row 3, W * C = 111 (odd): row0 = 5 puts the first input element at
    an even offset (it streams), row0 = 4 at an odd one (the generic kernel)."""
    rng = np.random.default_rng(22)
    w, c, b = 37, 3, 12 if not with_std else 10
    for row0, pairs_ok in ((5, True), (4, False)):
        tile = (16, row0, 6, 3)
        h16.check_embedding(eng, DEV, (13, w, c), 7, b, with_std, variants_for(c, b, with_std), tile=tile,
                            expect=expect_kernels(c, b, with_std, pairs_ok=pairs_ok), **h16.flat_kw(rng, 6, w, c, with_std))


# ---------------------------------------------------------------------------------------------- 2. the variants agree
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("b", DEPTHS)
def test_variants_agree(eng, shape, b):
    """Random full-range DNs on full tables: the default dispatch and every forced variant that is legal give identical bits."""
    h, w, c = shape
    rng = np.random.default_rng(300 + b + c)
    n = 9
    frames = [T(f, DEV) for f in full_range_frames(rng, n, shape, b)]
    icrf, diff = tables_bits(c, b)
    sd = [T(s, DEV) for s in make_stds(rng, n, shape)]
    for with_std in (False, True):
        kw = {k: (T(v, DEV) if isinstance(v, np.ndarray) else v) for k, v in h16.flat_kw(rng, h, w, c, with_std).items()}
        outs = {}
        for v in variants_for(c, b, with_std):
            plan = eng.plan_merge(frames, exposures(n), icrf, diff if with_std else None, sd if with_std else None, bit_depth=b, variant=v,
                                  want_sum_w=True, **kw)
            for o in plan.outputs.values():
                o.fill_(float("nan"))
            plan.launch()
            expect_kernels(c, b, with_std)(v, plan.kernels, h * w * c)
            outs[v] = plan.outputs
        for v, o in outs.items():
            for k in outs[0]:
                assert_same_bits(o[k], outs[0][k], f"{k} variant {v}")


# ---------------------------------------------------------------------------------------------- 3. against the arithmetic
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("b", DEPTHS)
def test_arithmetic(eng, shape, b):
    h16.check_arithmetic(eng, DEV, shape, 7, b, with_std=True)
    h16.check_arithmetic(eng, DEV, shape, 9, b, with_std=False, with_flat=True)
    h16.check_arithmetic(eng, DEV, shape, 32, b, with_std=True, with_flat=True, variant=2)
    h16.check_arithmetic(eng, DEV, shape, 2, b, with_std=True, variant=-1)


# ---------------------------------------------------------------------------------------------- 4. float32 outputs
@pytest.mark.parametrize("variant", [0, 2, -1])
def test_float32_outputs_are_the_cast_float64_outputs(eng, variant):
    rng = np.random.default_rng(11)
    shape, n, b = (13, 37, 3), 7, 10
    frames = [T(f, DEV) for f in full_range_frames(rng, n, shape, b)]
    icrf, diff = tables_bits(3, b)
    sd = [T(s, DEV) for s in make_stds(rng, n, shape)]
    o64 = eng.merge(frames, exposures(n), icrf, diff, sd, bit_depth=b, variant=variant)
    o32 = eng.merge(frames, exposures(n), icrf, diff, sd, bit_depth=b, variant=variant, out_dtype=F32)
    for k in ("val", "std"):
        assert o32[k].dtype == F32 and np.array_equal(o32[k].cpu().numpy(), o64[k].cpu().numpy().astype(np.float32))


# ---------------------------------------------------------------------------------------------- 5. hm_linearize_u16
@pytest.mark.parametrize("b", DEPTHS)
def test_linearize(eng, b):
    h16.check_linearize(eng, DEV, b, embedded=True)
    h16.check_linearize(eng, DEV, b, embedded=False)


# ---------------------------------------------------------------------------------------------- 7. Python surface on the device
def test_plan_graph_of_two_12_bit_plans(eng):
    rng = np.random.default_rng(31)
    n, b = 7, 12
    icrf, diff = tables_bits(3, b)
    plans, want = [], []
    for shape, with_std in (((13, 37, 3), False), ((8, 64, 3), True)):
        frames = [T(f, DEV) for f in full_range_frames(rng, n, shape, b)]
        sd = [T(s, DEV) for s in make_stds(rng, n, shape)] if with_std else None
        plans.append(eng.plan_merge(frames, exposures(n), icrf, diff if with_std else None, sd, bit_depth=b))
        p = eng.plan_merge(frames, exposures(n), icrf, diff if with_std else None, sd, bit_depth=b)
        p.launch()
        want.append(p.outputs)
    assert "tab=lds" in plans[0].kernels and "tab=mixed-wdwg" in plans[1].kernels
    graph = eng.PlanGraph(plans)
    for p in plans:
        for o in p.outputs.values():
            o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for p, w in zip(plans, want):
        for k in w:
            assert_same_bits(p.outputs[k], w[k], k)


def test_tiff_round_trip_into_plan_merge(eng, tmp_path):
    from camera_linearity_amd import tiff_io
    rng = np.random.default_rng(8)
    n, shape, b = 3, (9, 31, 3), 12
    frames = full_range_frames(rng, n, shape, b)
    back = []
    for i, f in enumerate(frames):
        assert tiff_io.imwrite(tmp_path / f"f{i}.tif", f)
        r = tiff_io.imread(tmp_path / f"f{i}.tif", tiff_io.IMREAD_UNCHANGED)
        assert r.dtype == np.uint16
        back.append(T(r, DEV))
    icrf, _ = tables_bits(3, b)
    plan = eng.plan_merge(back, exposures(n), icrf, bit_depth=b)
    assert plan.kernels.startswith("merge_u16_stream<tab=lds,bits=12,")
    plan.launch()
    want = h16.numpy_merge_u16(frames, b, exposures(n), icrf)
    np.testing.assert_allclose(plan.outputs["val"].cpu().numpy(), want["val"], rtol=h16.VAL_RTOL, atol=0)
