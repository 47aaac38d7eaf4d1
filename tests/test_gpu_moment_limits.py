"""The mean / std reductions (csrc/hm_stats.hip: k_stats, k_stats_final, k_pair_stats, k_pair_final, k_pairs_stats, k_pairs_stats_lds,
k_pairs_final; csrc/hm_pointwise.hip: k_thresholds; csrc/hm_stats_axis.hip: k_axis_thread, k_axis_row, k_axis_final, k_axis_final_tree,
k_axis_final2, k_axis_final2_tree) on the MI355X at
the limits of their ABI: the checks of tests/test_moment_limits_host.py - the reference, the derived bounds and every case live there - on
device tensors, plus the sizes at which a lane folds a 64-element block in mid-stream, a path only the device build has. Every test
asserts that the device symbol ran and the host one did not."""
import contextlib

import pytest

from camera_linearity_amd import _native as nat

import test_moment_limits_host as ml
from test_moment_limits_host import report_moment_maxima  # noqa: F401  (prints the observed maxima after this module too)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STD = pytest.mark.parametrize("weighted", [False, True])
CHAN, AXIS, AXIS2, PAIR, PAIRS = "hm_channel_statistics", "hm_axis_statistics", "hm_axis_statistics2", "hm_pair_statistics", "hm_pairs_statistics"


@contextlib.contextmanager
def on_device(*symbols):
    """Every one of `symbols` is called in the HIP library inside the block, none of them in the host library."""
    hip, host = nat.hip_lib.calls, nat.host_lib().calls
    before = {s: (hip[s], host[s]) for s in symbols}
    yield
    for s, (d, h) in before.items():
        assert hip[s] > d and host[s] == h, (s, hip[s] - d, host[s] - h)


@STD
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_channel_sizes(C_, weighted):
    with on_device(CHAN):
        for n in ml.channel_sizes(C_, weighted):
            ml.check_channel(DEV, n, C_, weighted)


@STD
@pytest.mark.parametrize("C_", [3, 4])
def test_channel_two_folds(C_, weighted):
    """2 x 12 582 912 + 3 x C x 37 elements: two mid-stream folds, both prefetch register sets, a ragged tail."""
    n = ml.TWO_FOLDS + 3 * C_ * 37
    assert ml.stream_depth(True, n, C_, 4 if weighted else 8)["folds"] == 4
    with on_device(CHAN):
        ml.check_channel(DEV, n, C_, weighted)


@STD
def test_channel_offset_view(weighted):
    with on_device(CHAN):
        ml.check_channel(DEV, 3 * 4099, 3, weighted, off8=True)


@STD
def test_channel_offset_family(weighted):
    """Mean 1e6, spread 1e-3 at the two-fold size."""
    with on_device(CHAN):
        ml.check_channel(DEV, 3 * 65599, 3, weighted, fam="offset")
        ml.check_channel(DEV, ml.TWO_FOLDS + 3 * 3 * 37, 3, weighted, fam="offset")


def test_channel_heavy_tailed():
    with on_device(CHAN):
        ml.check_channel_heavy(DEV)


def test_negative_stds():
    with on_device(CHAN, AXIS):
        ml.check_channel_negative(DEV)


def test_specials():
    with on_device(CHAN, AXIS):
        ml.check_specials(DEV)


def test_extreme_weights_mid_block():
    with on_device(AXIS, CHAN):
        ml.check_extreme_weights_mid_block(DEV)


@STD
@pytest.mark.parametrize("shape", list(ml.AXIS_THREAD), ids=str)
def test_axis_thread(shape, weighted):
    with on_device(AXIS):
        ml.check_axis(DEV, shape, weighted, ml.AXIS_THREAD[shape], with_err=ml.with_err_for(shape))


@STD
@pytest.mark.parametrize("shape", list(ml.AXIS_ROW) + list(ml.AXIS_ROW_LONG), ids=str)
def test_axis_row(shape, weighted):
    with on_device(AXIS):
        ml.check_axis(DEV, shape, weighted, {**ml.AXIS_ROW, **ml.AXIS_ROW_LONG}[shape], with_err=ml.with_err_for(shape))


@STD
def test_axis_offset_family_and_view(weighted):
    with on_device(AXIS):
        ml.check_axis(DEV, (1, 33280, 16), weighted, ml.AXIS_THREAD[(1, 33280, 16)], fam="offset")
        ml.check_axis(DEV, (1, 6000, 15), weighted, ml.AXIS_ROW[(1, 6000, 15)], fam="offset")
        ml.check_axis(DEV, (3, 200, 40), weighted, ml.AXIS_THREAD[(3, 200, 40)], off8=True)
        ml.check_axis(DEV, (1024, 33, 3), weighted, ml.AXIS_ROW[(1024, 33, 3)], off8=True)


def test_axis_heavy_tailed():
    with on_device(AXIS):
        ml.check_axis_heavy(DEV)


@STD
@pytest.mark.parametrize("shape", list(ml.AXIS2), ids=str)
def test_axis2(shape, weighted):
    with on_device(AXIS2):
        ml.check_axis2(DEV, shape, weighted, ml.AXIS2[shape])


@pytest.mark.parametrize("SX,SY", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("C_", [1, 3, 4])
def test_pair_sizes(C_, SX, SY):
    with on_device(PAIR):
        for k, n in enumerate(ml.pair_sizes(C_, SX or SY)):
            ml.check_pair(DEV, n, C_, SX, SY, (0.1, 0.1, 1.0, 7.3, 1.0)[k])


@pytest.mark.parametrize("std", [True, False])
def test_pair_two_folds(std):
    """The two-fold size of the per-pair kernel: 32 iterations of UN = 2 chunks with stds, 16 of UN = 4 without, twice, and a tail."""
    n = ml.TWO_FOLDS + 3 * 3 * 37
    assert ml.stream_depth(True, n, 3, 2 if std else 4)["folds"] == 4
    with on_device(PAIR):
        ml.check_pair(DEV, n, 3, std, std, 7.3)


def test_pair_offset_view():
    with on_device(PAIR):
        ml.check_pair(DEV, 3 * 4099, 3, True, True, 7.3, off8=True)


def test_pair_heavy_tailed():
    with on_device(PAIR):
        ml.check_pair_heavy(DEV)


def test_pair_specials():
    with on_device(PAIR):
        ml.check_pair_specials(DEV)
        ml.check_pair_one_special_lane(DEV)


@pytest.mark.parametrize("with_std", [False, True])
@pytest.mark.parametrize("n,what,r", ml.PAIRS_SIZES, ids=[w for _, w, _ in ml.PAIRS_SIZES])
def test_pairs_sizes(n, what, r, with_std):
    with on_device(PAIRS):
        ml.check_pairs_size(DEV, n, r, with_std)


@pytest.mark.parametrize("with_std", [False, True])
def test_pairs_block_fold(with_std):
    """3 145 728 + 2 x 98 304 + 37 C elements per frame: the block fold of k_pairs_stats_lds, two more iterations, a tail."""
    n = 3145728 + 2 * ml.IT + 37 * 3
    assert ml.stream_depth(True, n, 3, 2, per=64)["folds"] == 3
    with on_device(PAIRS):
        ml.check_pairs(DEV, 3, 3, n, 3, with_std, ["lds1"])


@pytest.mark.parametrize("frames,pairs,with_std,expect", ml.PAIRS_LIMITS)
def test_pairs_limits(frames, pairs, with_std, expect):
    with on_device(PAIRS):
        ml.check_pairs(DEV, frames, pairs, ml.IT + 64 * 3 + 3, 3, with_std, expect)


def test_pairs_unaligned_frame():
    with on_device(PAIRS):
        ml.check_pairs(DEV, 3, 3, ml.IT + 64 * 3 + 3, 3, True, ["plain"], off8_frame=1)


@pytest.mark.parametrize("with_std", [False, True])
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_pairs_thresholds(C_, with_std):
    thr = ml.THRESHOLDS[C_]
    with on_device(PAIRS):
        ml.check_pairs(DEV, 4, 2, ml.THR_N, C_, with_std, ["lds2"], thr, expect_fused=True, fam="pairs thresholds")
        ml.check_pairs(DEV, 4, 3, 12 * 250, C_, with_std, ["lds2"], thr, expect_fused=False, fam="pairs thresholds")
        ml.check_pairs(DEV, 4, 3, ml.THR_N, C_, with_std, ["plain"], thr, off8_frame=2, expect_fused=False, fam="pairs thresholds")
        ml.check_pairs(DEV, 5, 2, ml.THR_N, C_, with_std, ["plain"], thr, expect_fused=False, fam="pairs thresholds")


def test_thresholds_keep_values_on_a_limit():
    with on_device(PAIRS):
        ml.check_thresholds_on_a_limit(DEV)


def test_status_codes():
    with on_device(CHAN, AXIS, AXIS2, PAIR, PAIRS):
        assert ml.check_status(DEV) >= 48
