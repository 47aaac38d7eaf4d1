"""hm_pairs_statistics_dn on the MI355X (csrc/hm_stats_dn.hip: k_pairs_dn_table, k_pairs_stats_dn_lds, k_pairs_stats_dn_wave): the checks of
tests/test_pairs_stats_dn_host.py - the oracle, the inputs and every case live there - on device tensors, bit for bit against
N x hm_linearize_* + hm_pairs_statistics on the same device. Every test asserts that the device symbol ran and the host one did not."""
import pytest
import torch

from camera_linearity_amd import engine

import test_pairs_stats_dn_host as dn
from test_gpu_stats_limits import on_device

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENTRY = "hm_pairs_statistics_dn"
STD = pytest.mark.parametrize("with_std", [False, True])


@STD
def test_parent_forms_agree(with_std):
    with on_device("hm_pairs_statistics"):
        dn.check_parent_forms(DEV, with_std)


@pytest.mark.parametrize("with_thr", [False, True])
@STD
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
@pytest.mark.parametrize("size", dn.SIZES)
def test_shapes(size, C_, with_std, with_thr):
    with on_device(ENTRY):
        dn.check_shapes(DEV, size, C_, with_std, with_thr)


@STD
@pytest.mark.parametrize("n_frames,n_pairs", dn.SHAPES)
def test_frames_pairs(n_frames, n_pairs, with_std):
    with on_device(ENTRY):
        dn.check_frames_pairs(DEV, n_frames, n_pairs, with_std)


@STD
@pytest.mark.parametrize("bits", [8, 12])
def test_alignment(bits, with_std):
    with on_device(ENTRY):
        dn.check_alignment(DEV, bits, with_std)


@pytest.mark.parametrize("bits,C_,with_std", [(8, 3, True), (10, 3, True), (12, 3, True), (12, 3, False), (12, 4, False), (16, 3, True), (16, 1, False)])
def test_depths(bits, C_, with_std):
    with on_device(ENTRY):
        dn.check_depth(DEV, bits, C_, with_std)


@pytest.mark.parametrize("bits", [8, 12])
def test_zero_std(bits):
    with on_device(ENTRY):
        dn.check_zero_std(DEV, bits)


@STD
def test_stray_bits(with_std):
    with on_device(ENTRY):
        dn.check_stray_bits(DEV, with_std)


@pytest.mark.parametrize("bits,with_std", [(8, True), (10, True), (12, True), (12, False), (16, False)])
def test_variants(bits, with_std):
    with on_device(ENTRY):
        dn.check_variants(DEV, bits, with_std)


def test_status():
    with on_device(ENTRY):
        dn.check_status(DEV)


def test_value_errors():
    dn.check_value_errors(DEV)


@STD
def test_series(with_std):
    with on_device(ENTRY):
        dn.check_series(DEV, with_std)


def test_series_errors():
    dn.check_series_errors(DEV)


@pytest.mark.parametrize("bits,with_std", [(8, True), (12, True), (12, False)])
def test_graph_replay(bits, with_std):
    """The entry neither allocates nor synchronises: a PlanGraph records it (table kernel, statistics kernels, final fold) and its replay
    on fresh DNs gives the eager result."""
    C_, n, nf = 3, dn.N_BIG, 7
    icrf, diff, std = dn.tables(bits, C_)
    pairs, thr = dn.pair_list(nf, 21), dn.limits(bits, C_)
    first = [dn.T(f, DEV) for f in dn.dn_frames(bits, C_, n, nf)]
    second = [dn.T(f, DEV) for f in dn.dn_frames(bits, C_ + 1, n, nf)]                      # other DNs of the same size
    second = [s.reshape(-1)[:n].reshape(first[0].shape).contiguous() for s in second]
    kw = dict(bit_depth=None if bits == 8 else bits)
    with on_device(ENTRY):
        plan = engine.PairsDnPlan(first, pairs, icrf, diff if with_std else None, std if with_std else None, thr, **kw)
        graph = engine.PlanGraph([plan])
        for f, s in zip(plan.frames, second):
            f.copy_(s)
        plan.outputs["stats"].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        replayed = plan.outputs["stats"].clone()
        eager = engine.PairsDnPlan(second, pairs, icrf, diff if with_std else None, std if with_std else None, thr, **kw)
        eager.launch()
        torch.cuda.synchronize()
    assert torch.equal(replayed.view(torch.int64), eager.outputs["stats"].view(torch.int64))
    assert not torch.equal(replayed, torch.full_like(replayed, -1.0))
