"""hm_pairs_minmax_dn / hm_pairs_histogram_dn on the MI355X (csrc/hm_stats_hist_dn.hip: k_pairs_hist_dn, k_pairs_minmax_dn; csrc/hm_stats_dn.hip:
k_pairs_dn_table): the checks of tests/test_pairs_hist_dn_host.py - the oracle, the inputs and every case live there - on device tensors,
against the NumPy reference and against N x hm_linearize_* + hm_pairs_histogram / hm_pairs_minmax on the same device. Every test asserts
that the device symbols ran and the host ones did not."""
import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat

import test_pairs_hist_dn_host as hd
import test_pairs_stats_dn_host as dn
from test_gpu_stats_limits import on_device
from test_stats_limits_host import report_observed_maxima  # noqa: F401  (prints the observed maxima after this module too)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STD = pytest.mark.parametrize("with_std", [False, True])
BOTH = ("hm_pairs_histogram_dn", "hm_pairs_minmax_dn")


@STD
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
@pytest.mark.parametrize("name,npix", hd.SIZES)
def test_sizes(name, npix, C_, with_std):
    with on_device(*BOTH):
        hd.check_sizes(DEV, npix, C_, with_std)


@STD
@pytest.mark.parametrize("n_frames,n_pairs,bins", hd.FRAMES_PAIRS)
def test_frames_pairs(n_frames, n_pairs, bins, with_std):
    with on_device(*BOTH):
        hd.check_frames_pairs(DEV, n_frames, n_pairs, bins, with_std)


@STD
@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_depths(bits, with_std):
    with on_device(*BOTH):
        hd.check_depth(DEV, bits, with_std)


@STD
@pytest.mark.parametrize("bits", [8, 12])
@pytest.mark.parametrize("bins", hd.BINS)
def test_bins(bins, bits, with_std):
    with on_device(*BOTH):
        hd.check_bins(DEV, bins, bits, with_std)


@STD
@pytest.mark.parametrize("bits", [8, 12])
def test_misaligned(bits, with_std):
    with on_device(*BOTH):
        hd.check_misaligned(DEV, bits, with_std)


@STD
def test_stray_bits(with_std):
    with on_device(*BOTH):
        hd.check_stray_bits(DEV, with_std)


@pytest.mark.parametrize("bits", [8, 12])
def test_zero_std(bits):
    with on_device(*BOTH):
        hd.check_zero_std(DEV, bits)


@STD
def test_specials(with_std):
    with on_device(*BOTH):
        hd.check_specials(DEV, with_std)


@STD
def test_masks(with_std):
    with on_device(*BOTH):
        hd.check_masks(DEV, with_std)


@STD
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("lo,hi,bins,C_", hd.EDGE_SETS)
def test_edges(lo, hi, bins, C_, kind, with_std):
    with on_device(*BOTH):
        hd.check_edges(DEV, lo, hi, bins, C_, kind, with_std)


def test_flat_edges():
    with on_device("hm_pairs_histogram_dn"):
        hd.check_flat_edges(DEV)


def test_status():
    with on_device(*BOTH):
        hd.check_status(DEV)


@STD
@pytest.mark.parametrize("bits", [8, 12])
def test_engine(bits, with_std):
    with on_device(*BOTH):
        hd.check_engine(DEV, bits, with_std)


def test_value_errors():
    hd.check_value_errors(DEV)


@STD
def test_series(with_std):
    with on_device(*BOTH):
        hd.check_series(DEV, with_std)


def test_series_errors():
    hd.check_series_errors(DEV)


@pytest.mark.parametrize("bits,with_std,bins", [(8, True, 256), (12, True, 64), (12, False, 256)])
def test_graph_replay(bits, with_std, bins):
    """The entry neither allocates nor synchronises: one torch.cuda.graph records hm_pairs_histogram_dn (table kernel, histogram kernels,
    column sums) with a caller-held workspace and fixed edges, and its replay on fresh DNs gives the eager counts."""
    C_, npix, nf = 3, 4001, 7
    tabs, thr = dn.tables(bits, C_), dn.limits(bits, C_)
    pairs = hd.ratio_pairs(nf, 15)
    first = [dn.T(f, DEV) for f in hd.frames_of(bits, C_, npix, nf)]
    second = [dn.T(f, DEV) for f in reversed(hd.frames_of(bits, C_, npix, nf))]               # other DNs of the same size
    edges = hd.linspace_edges(np.tile([-0.6, 0.6], (15, 2, C_, 1)), bins)
    lib = nat.hip_lib
    with torch.cuda.device(DEV):
        a = hd.DnArgs(DEV, first, tabs, pairs, with_std)
        lo, hi = hd.ph.limits(thr, C_)
        e = dn.T(edges, DEV)
        out = torch.full((15 * 2 * C_ * bins,), -1.0, dtype=torch.float64, device=DEV)
        ws = torch.empty(lib.hm_pairs_histogram_dn_workspace_bytes(15, bins, C_, bits) // 8 + 1, dtype=torch.float64, device=DEV)

        def launch():
            rc = lib.hm_pairs_histogram_dn(a.fp, nf, bits, a.tp(0), a.tp(1), a.tp(2), a.pi, a.pj, a.pm, 15, npix * C_, C_, 7, lo, hi, e.data_ptr(), bins, 0,
                                           out.data_ptr(), ws.data_ptr(), nat.current_stream_ptr(torch.device(DEV)))
            assert rc == nat.HM_OK
        with on_device("hm_pairs_histogram_dn"):
            launch()                                                                            # (the once-per-process LDS limit is set here)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                launch()
            for f, s in zip(first, second):
                f.copy_(s)
            out.fill_(-1.0)
            graph.replay()
            torch.cuda.synchronize()
            replayed = out.clone()
            out.fill_(-1.0)
            launch()
            torch.cuda.synchronize()
    if with_std:
        case = hd.Case(DEV, [f.cpu().numpy() for f in second], tabs, pairs, True, bins, (-0.6, 0.6), thr=thr, what="graph replay")
        for (p, k, c), ref in case.hist.items():
            hd.same_weighted(DEV, replayed.cpu().numpy().reshape(15, 2, C_, bins)[p, k, c], out.cpu().numpy().reshape(15, 2, C_, bins)[p, k, c], ref,
                             "replayed against eager", "pairs dn replay")
    else:
        assert torch.equal(replayed, out)
    assert not torch.equal(replayed, torch.full_like(replayed, -1.0)) and float(replayed.sum()) > 0
