"""Hot-pixel filtering in the fused merge on uint16 DN frames (hm_merge_u16_darks) on the GPU: the checks of
tests/test_merge_u16_darks_host.py - pre-filtered equality bit for bit against hm_merge_u16 on frames filtered with the oracle's median, the
embedding of an 8-bit stack with uint8 maps against hm_merge, the NumPy restatement - on merge_u16_scan_hot + merge_u16_patch_hot, with
plan.kernels asserting which form of the pass ran.

Shapes are the smallest that cross every boundary: (13, 37, 3) wave groups plus a generic tail and an odd W C (the scan's scalar path on a
row tile), (8, 64, 4) whole groups and the aligned 16-byte scan, (3, 43, 1) H = 3 where k = 7 reflects past both edges, (48, 456, 3) 128
elements past one 65 536-element scan piece with hot elements at 65 535 and 65 536. Depths 9, 12, 16; N = 1, 7, 9, 32; k = 3, 5, 7.
Densities: about 1 % (the queue), 60 %, 1 % with the smallest legal workspace (one entry: overflow), and no workspace (queue=0). The
recommended workspace of a tile of fewer than 4096 elements has one queue entry per element and cannot overflow, so 60 % on the small
shapes is a full queue; the recommended 25 % queue overflows on (48, 456, 3) at 60 % (the first scan piece alone) and on (96, 456, 3) at
about 30 % (each of the two whole scan pieces fits, both do not: a queue partly filled before the flag is raised). Every legal streaming
variant runs with one map mix; row tiles with their halo; a relaunch with the maps overwritten in place, also through a hipGraph replay."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_merge_u16_host as h16  # noqa: E402
import test_merge_u16_darks_host as hd  # noqa: E402
from test_merge_u16_darks_host import BIG, DEPTHS, SHAPES  # noqa: E402
from test_merge_u16_host import F32  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from camera_linearity_amd import engine
    assert torch.cuda.is_available()
    return engine


def variants_for(c, b, with_std):
    """The default and every forced variant that is legal: -1 one element per thread, 1 tables in LDS, 2 in global memory, 3 split."""
    return (-1, 2, 0) + ((1,) if h16.fits_lds(c, b, with_std) else ()) + ((3,) if h16.mixed_placement(c, b, with_std) else ())


def expect_pass(b, k, with_std, f32=False):
    """plan.kernels: hm_merge_u16's kernels, then the scan and the patch kernel - or the patch kernel alone, queue=0, without a workspace."""
    def expect(v, names, workspace):
        parts = names.split(" + ")
        tail = f"bits={b},std={int(with_std)},k={k}"
        out = ",out=f32" if f32 else ""
        if workspace == "none":
            assert parts[-1] == f"merge_u16_patch_hot<{tail},queue=0{out}>" and "merge_u16_scan_hot" not in parts, names
            head = parts[:-1]
        else:
            assert parts[-2:] == ["merge_u16_scan_hot", f"merge_u16_patch_hot<{tail}{out}>"], names
            head = parts[:-2]
        assert head and all(p.startswith(("merge_u16_stream<", "merge_u16_generic<")) for p in head), names
        if v == -1:
            assert len(head) == 1 and head[0].startswith("merge_u16_generic<"), names
    return expect


# ---------------------------------------------------------------------------------------------- 1. pre-filtered equality
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("b", DEPTHS)
def test_prefiltered(eng, shape, b):
    for n, k, with_std in ((7, 3, False), (9, 5, True), (7, 7, True), (9, 3, True)):
        hd.check_prefiltered(eng, DEV, shape, n, b, k, with_std, expect=expect_pass(b, k, with_std))


@pytest.mark.parametrize("n", [1, 7, 9, 32])
def test_frame_counts(eng, n):
    for b, k, with_std in ((12, 3, True), (9, 5, False), (16, 7, True)):
        hd.check_prefiltered(eng, DEV, (13, 37, 3), n, b, k, with_std, want_sum_w=True, expect=expect_pass(b, k, with_std))
    hd.check_prefiltered(eng, DEV, (8, 64, 4), n, 12, 3, True, workspace="none", expect=expect_pass(12, 3, True))


@pytest.mark.parametrize("density,workspace", [(0.01, "rec"), (0.6, "rec"), (0.01, "min"), (0.01, "none"), (0.6, "none")],
                         ids=["queue", "queue-dense", "overflow-min", "no-workspace", "no-workspace-dense"])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_densities_and_workspaces(eng, density, workspace, k):
    for shape, b, with_std in (((13, 37, 3), 12, True), ((8, 64, 4), 16, False), ((3, 43, 1), 9, True)):
        hd.check_prefiltered(eng, DEV, shape, 7, b, k, with_std, density=density, workspace=workspace, expect=expect_pass(b, k, with_std))


@pytest.mark.parametrize("workspace", ["rec", "min", "none"])
def test_two_scan_pieces(eng, workspace):
    """65 664 elements: hot elements at 65 535 and 65 536, the last of the first scan piece and the first of the second."""
    hd.check_prefiltered(eng, DEV, BIG, 7, 12, 3, True, workspace=workspace, expect=expect_pass(12, 3, True))
    hd.check_prefiltered(eng, DEV, BIG, 9, 16, 5, False, workspace=workspace, density=0.002, expect=expect_pass(16, 5, False))


def test_recommended_queue_overflows(eng):
    """More hot elements than the recommended workspace's quarter: the scan raises the flag - at once, or after one piece was queued - and
    the patch kernel goes over the whole tile."""
    hd.check_overflowing_recommended_queue(eng, DEV, expect=lambda v, names, ws: "merge_u16_scan_hot + merge_u16_patch_hot<" in names)


@pytest.mark.parametrize("with_std", [False, True], ids=["val", "std"])
@pytest.mark.parametrize("b", DEPTHS)
def test_every_streaming_variant(eng, b, with_std):
    """The patch does not depend on where the streaming kernel keeps its tables: every legal variant with one map mix."""
    for shape in ((13, 37, 3), (8, 64, 4)):
        c = shape[2]
        names = hd.check_prefiltered(eng, DEV, shape, 7, b, 3, with_std, variants=variants_for(c, b, with_std), expect=expect_pass(b, 3, with_std))
        assert names[2].startswith("merge_u16_stream<tab=global,") and names[-1].startswith("merge_u16_generic<")


@pytest.mark.parametrize("with_std", [False, True], ids=["val", "std"])
@pytest.mark.parametrize("out_dtype", [torch.float64, F32], ids=["f64", "f32"])
def test_flat_field_outputs_and_sum_of_weights(eng, with_std, out_dtype):
    f32 = out_dtype == F32
    for shape, b, k in (((13, 37, 3), 12, 3), ((8, 64, 4), 16, 5), ((3, 43, 1), 9, 7)):
        for workspace in ("rec", "none"):
            hd.check_prefiltered(eng, DEV, shape, 7, b, k, with_std, workspace=workspace, with_flat=True, want_sum_w=True, out_dtype=out_dtype,
                                 expect=expect_pass(b, k, with_std, f32))
            hd.check_prefiltered(eng, DEV, shape, 7, b, k, with_std, workspace=workspace, out_dtype=out_dtype, expect=expect_pass(b, k, with_std, f32))


@pytest.mark.parametrize("workspace", ["rec", "min", "none"])
def test_sum_of_weights_only(eng, workspace):
    for shape, b, k in (((13, 37, 3), 12, 3), ((8, 64, 4), 9, 5), ((3, 43, 1), 16, 7)):
        names = hd.check_prefiltered(eng, DEV, shape, 9, b, k, False, workspace=workspace, want_val=False, want_sum_w=True,
                                     expect=expect_pass(b, k, False))
        assert names[0].startswith("merge_u16_generic<")


# ---------------------------------------------------------------------------------------------- row tiles
@pytest.mark.parametrize("tile", [(16, 5, 6, 3), (16, 4, 6, 3), (16, 0, 5, 0), (16, 11, 5, 9)], ids=["even-offset", "odd-offset", "top", "bottom"])
@pytest.mark.parametrize("workspace", ["rec", "none"])
def test_row_tiles(eng, tile, workspace):
    """Rows of a 16-row image with W C = 111 (odd) from buffers that start at row 3: row0 = 5 puts the first input element at an even
    offset, row0 = 4 at an odd one (the scan's scalar path, the generic kernel); a tile touching row 0 and one touching the last row."""
    for with_std in (False, True):
        hd.check_prefiltered(eng, DEV, (16, 37, 3), 7, 12, 3, with_std, workspace=workspace, tile=tile, with_flat=True,
                             expect=expect_pass(12, 3, with_std))
    if tile[1] > 3:
        for k in (5, 7):
            hd.check_prefiltered(eng, DEV, (16, 37, 3), 7, 12, k, True, workspace=workspace, tile=(tile[0], tile[1], tile[2], tile[1] - k // 2),
                                 expect=expect_pass(12, k, True))


def test_row_tile_one_halo_row_short(eng):
    rng = np.random.default_rng(4)
    n, b = 3, 12
    icrf, _ = h16.tables_bits(3, b)
    frames = [h16.T(f, DEV) for f in h16.full_range_frames(rng, n, (12, 37, 3), b)]
    dark = h16.T(rng.integers(0, 4096, size=(12, 37, 3)).astype(np.uint16), DEV)
    kw = dict(darks=[None, dark, dark], dark_min=[4096, 3000, 3000], bit_depth=b, height=16, rows=6)
    for k in (3, 5, 7):
        r = k // 2
        eng.plan_merge(frames, h16.exposures(n), icrf, median_k=k, row0=4 + r, buf_row0=4, **kw)
        with pytest.raises(ValueError, match="geometry"):
            eng.plan_merge(frames, h16.exposures(n), icrf, median_k=k, row0=4 + r - 1, buf_row0=4, **kw)
    with pytest.raises(ValueError, match="geometry"):                      # rows [9, 15) of 16 from buffers that end at row 16 - 1
        eng.plan_merge([f[:11] for f in frames], h16.exposures(n), icrf, median_k=3, row0=9, buf_row0=4, darks=[None, dark[:11], dark[:11]],
                       dark_min=[4096, 3000, 3000], bit_depth=b, height=16, rows=6)


# ---------------------------------------------------------------------------------------------- 2. embedding, 3. arithmetic
@pytest.mark.parametrize("b", DEPTHS)
@pytest.mark.parametrize("workspace", ["rec", "none"])
def test_embedding(eng, b, workspace):
    rng = np.random.default_rng(b)
    for shape, n, k, with_std in (((13, 37, 3), 7, 3, True), ((8, 64, 4), 9, 5, False), ((3, 43, 1), 7, 7, True), ((13, 37, 3), 32, 3, False)):
        h, w, c = shape
        names = hd.check_embedding(eng, DEV, shape, n, b, k, with_std, workspace=workspace, want_sum_w=True)
        assert ("queue=0" in names) == (workspace == "none") and f"merge_u16_patch_hot<bits={b},std={int(with_std)},k={k}" in names
        hd.check_embedding(eng, DEV, shape, n, b, k, with_std, workspace=workspace, out_dtype=F32, **h16.flat_kw(rng, h, w, c, with_std))


@pytest.mark.parametrize("b", DEPTHS)
def test_arithmetic(eng, b):
    hd.check_arithmetic(eng, DEV, (13, 37, 3), 7, b, 3, with_std=True)
    hd.check_arithmetic(eng, DEV, (8, 64, 4), 9, b, 5, with_std=False, with_flat=True)
    hd.check_arithmetic(eng, DEV, (3, 43, 1), 2, b, 7, with_std=True, with_flat=True, workspace="none")
    hd.check_arithmetic(eng, DEV, (13, 37, 3), 32, b, 3, with_std=True, with_flat=True)


# ---------------------------------------------------------------------------------------------- relaunch
def test_relaunch_with_new_maps(eng):
    hd.check_relaunch(eng, DEV)


def test_relaunch_through_plan_graph(eng):
    """The recorded launches (streaming kernels, scan, patch) replayed after the maps changed in place: the counters are zeroed by the
    recorded kernels themselves, so nothing of the first launch's queue survives."""
    graphs = []

    def replay(plan):
        graphs.append(eng.PlanGraph([plan], warmup=False))
        for o in plan.outputs.values():
            o.fill_(float("nan"))
        graphs[0].replay()
        torch.cuda.synchronize()
    hd.check_relaunch(eng, DEV, launch_again=replay)
    assert graphs
