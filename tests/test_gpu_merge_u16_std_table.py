"""The fused merge of 9- to 16-bit cameras with the stds from the per-DN STD table (hm_merge_u16_std_table) on the GPU: the check
functions of tests/test_merge_u16_std_table_host.py - equality of bit patterns with engine.merge(..., stds=materialised, bit_depth=b) on the
device and with the host build - on the LUT instantiations of merge_u16_stream / merge_u16_generic / merge_u16_patch_hot, with plan.kernels
asserting the placement that ran.

Shapes are the smallest that cross every boundary: (13, 37, 3) is 11 wave groups plus a generic tail with an odd W C, (8, 64, 4) whole
groups only; (48, 456, 3) is 128 elements past one 65 536-element scan piece. Depths 9, 10, 12, 16 and, for C = 3 and 4, the largest depth
whose tables fit in LDS (11) and the first that does not (12): every placement (lds, mixed-wdwdg, mixed-wdw, global) runs."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_merge_u16_std_table_host as ht  # noqa: E402
from test_merge_u16_host import FIT, assert_same_bits, full_range_frames, mixed_placement, tables_bits  # noqa: E402
from test_merge_u16_std_table_host import F32, F64, FRAME_COUNTS, T, TILES, exposures, std_table  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from camera_linearity_amd import engine
    assert torch.cuda.is_available()
    return engine


@pytest.fixture(scope="module")
def heng():
    from camera_linearity_amd.measurand import _HOST_ENGINE
    return _HOST_ENGINE


def variants_for(c, b):
    """The default and every forced variant that is legal for a std call: -1 one element per thread, 1 LDS, 2 global memory, 3 split."""
    return (-1, 0, 2) + ((1,) if b <= FIT[(c, True)] else ()) + ((3,) if mixed_placement(c, b, True) else ())


def expect_placement(c, b):
    def expect(v, names, n_elems):
        parts = names.split(" + ")
        assert all("std=lut" in p for p in parts), names
        if v == -1:
            assert len(parts) == 1 and parts[0].startswith("merge_u16_generic<"), names
            return
        assert parts[0].startswith(f"merge_u16_stream<tab={ht.table_placement(c, b, v)},bits={b},C={c},std=lut,"), names
        assert (len(parts) == 2 and parts[1].startswith("merge_u16_generic<")) if n_elems % 128 else len(parts) == 1, names
    return expect


@pytest.mark.parametrize("shape", [(13, 37, 3), (8, 64, 4)], ids=str)
@pytest.mark.parametrize("b", [9, 10, 11, 12, 16])
def test_every_variant(eng, heng, shape, b):
    c = shape[2]
    assert FIT[(c, True)] == 11                                   # 11: the largest depth that fits in LDS, 12: the first that does not
    out = ht.check_table(eng, DEV, shape, 7, b, variants=variants_for(c, b), expect=expect_placement(c, b))
    host = ht.check_table(heng, None, shape, 7, b)[0][1]
    for v, (names, got) in out.items():
        for key in host:
            assert_same_bits(got[key].cpu(), host[key], f"{key}: device against host build, variant={v} {names}")


@pytest.mark.parametrize("n", FRAME_COUNTS)
def test_frame_counts(eng, n):
    ht.check_table(eng, DEV, (13, 37, 3), n, 12, variants=(0, -1), expect=expect_placement(3, 12))


@pytest.mark.parametrize("out_dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("b", [10, 12, 13, 16])
def test_flat_field_outputs_and_sum_of_weights(eng, heng, out_dtype, b):
    out = ht.check_table(eng, DEV, (13, 37, 3), 7, b, with_flat=True, want_sum_w=True, out_dtype=out_dtype, other=(heng, None),
                         expect=expect_placement(3, b))
    assert ("out=f32" in out[0][0]) == (out_dtype == F32) and "flat=1,sum_w=1" in out[0][0]


@pytest.mark.parametrize("tile,wc", TILES, ids=["even-offset", "odd-offset"])
def test_row_tiles(eng, heng, tile, wc):
    w, c = wc
    out = ht.check_table(eng, DEV, (tile[0] - tile[3], w, c), 7, 12, variants=(0, 2), tile=tile, with_flat=True, want_sum_w=True, other=(heng, None))
    assert out[0][0].startswith("merge_u16_stream<" if tile[1] % 2 else "merge_u16_generic<")      # W C = 111: an odd row0 - buf_row0 breaks the pair rule


def expect_hot(names, b, k, hot_queue):
    parts = names.split(" + ")
    if hot_queue:
        assert parts[-2:] == ["merge_u16_scan_hot", f"merge_u16_patch_hot<bits={b},std=lut,k={k}>"], names
    else:
        assert parts[-1] == f"merge_u16_patch_hot<bits={b},std=lut,k={k},queue=0>" and "merge_u16_scan_hot" not in parts, names


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("hot_queue", [True, False], ids=["queue", "no-queue"])
@pytest.mark.parametrize("density", [0.01, 1.0])
@pytest.mark.parametrize("b", [9, 12])
def test_hot_pixels(eng, b, density, hot_queue, k):
    expect_hot(ht.check_table_hot(eng, DEV, (13, 37, 3), 7, b, k, density=density, hot_queue=hot_queue), b, k, hot_queue)


def test_hot_pixels_second_scan_piece(eng):
    expect_hot(ht.check_table_hot(eng, DEV, (48, 456, 3), 7, 12, 3, density=0.01), 12, 3, True)


@pytest.mark.parametrize("hot_queue", [True, False], ids=["queue", "no-queue"])
def test_hot_pixels_relaunch(eng, hot_queue):
    """One plan launched twice: the recorded counters are zeroed by the call's own first kernel, the bits are the same."""
    ht.check_table_hot(eng, DEV, (8, 64, 4), 9, 12, 3, density=0.05, hot_queue=hot_queue, relaunch=lambda plan: plan.launch())


def test_plan_graph_replay(eng):
    """A hipGraph replay of a table plan (streaming kernel, tail, scan, patch) equals its direct launch."""
    graphs = []

    def replay(plan):
        graphs.append(eng.PlanGraph([plan], warmup=False))
        for o in plan.outputs.values():
            o.fill_(float("nan"))
        graphs[-1].replay()
        torch.cuda.synchronize()
    ht.check_table_hot(eng, DEV, (13, 37, 3), 7, 12, 3, density=0.05, relaunch=replay)
    assert graphs


# ---------------------------------------------------------------------------------------------- MergePipeline(bit_depth=...)
def _stacks(count, n, shape, b):
    rng = np.random.default_rng(909)
    return [full_range_frames(rng, n, shape, b) for _ in range(count)]


def test_pipeline_std_table(eng):
    from camera_linearity_amd.pipeline import MergePipeline
    n, shape, b = 7, (13, 37, 3), 12
    icrf, diff = tables_bits(3, b)
    table = std_table(3, b)
    stacks = _stacks(3, n, shape, b)
    pipe = MergePipeline(n, shape[0], shape[1], exposures(n), icrf, diff, channels=3, device=DEV, bit_depth=b, std_table=table)
    for s in pipe.slots:
        assert s.h_stds is None and s.d_stds is None and s.plan._entry == "hm_merge_u16_std_table"
        assert all(f.dtype == torch.uint16 for f in s.h_frames + s.d_frames)
    got = pipe.merge_many(stacks)
    assert len(got) == 3
    for frames, (val, std) in zip(stacks, got):
        want = eng.merge_u16_std_table([T(f, DEV) for f in frames], exposures(n), icrf, diff, table, bit_depth=b)
        assert_same_bits(torch.from_numpy(val), want["val"].cpu(), "val")
        assert_same_bits(torch.from_numpy(std), want["std"].cpu(), "std")


def test_pipeline_uint16_value_only_and_with_std(eng):
    from camera_linearity_amd.pipeline import MergePipeline
    n, shape, b = 7, (13, 37, 3), 12
    icrf, diff = tables_bits(3, b)
    stacks = _stacks(3, n, shape, b)
    rng = np.random.default_rng(5)
    stds = [[0.004 * (1 + rng.random(shape)) for _ in range(n)] for _ in stacks]
    pipe = MergePipeline(n, shape[0], shape[1], exposures(n), icrf, channels=3, device=DEV, bit_depth=b)
    assert all(s.plan._entry == "hm_merge_u16" and s.h_stds is None for s in pipe.slots)
    for frames, (val, std) in zip(stacks, pipe.merge_many(stacks)):
        want = eng.merge([T(f, DEV) for f in frames], exposures(n), icrf, bit_depth=b)
        assert std is None
        assert_same_bits(torch.from_numpy(val), want["val"].cpu(), "val")
    pipe = MergePipeline(n, shape[0], shape[1], exposures(n), icrf, diff, channels=3, with_std=True, device=DEV, bit_depth=b)
    assert all(s.plan._entry == "hm_merge_u16" and s.h_stds[0].dtype == F64 for s in pipe.slots)
    for frames, sd, (val, std) in zip(stacks, stds, pipe.merge_many(stacks, stds)):
        want = eng.merge([T(f, DEV) for f in frames], exposures(n), icrf, diff, [T(s, DEV) for s in sd], bit_depth=b)
        assert_same_bits(torch.from_numpy(val), want["val"].cpu(), "val")
        assert_same_bits(torch.from_numpy(std), want["std"].cpu(), "std")
    with pytest.raises(ValueError, match="std_dtype"):
        MergePipeline(n, shape[0], shape[1], exposures(n), icrf, diff, with_std=True, std_dtype=F32, device=DEV, bit_depth=b)
