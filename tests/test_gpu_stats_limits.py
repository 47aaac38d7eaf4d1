"""The histogram and min / max kernels (csrc/hm_stats_hist.hip: k_hist, k_hist_final, k_minmax, k_minmax_final), the ROI mean
(csrc/hm_corrections.hip: k_roi_partial, k_roi_final) and the standalone hot-pixel filter (k_hot_filter, k_hot_filter_burst,
wave_median, lane_median) on the MI355X at the limits of their ABI: the checks of tests/test_stats_limits_host.py - the references, the
derived bounds and every case live there - on device tensors. Every test asserts that the device symbol ran and the host one did not."""
import contextlib

import pytest

from camera_linearity_amd import _native as nat

import test_stats_limits_host as sl
from test_stats_limits_host import report_observed_maxima  # noqa: F401  (prints the observed maxima after this module too)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STD = pytest.mark.parametrize("use_std", [False, True])
HIST = ("hm_channel_histogram",)
ROI = ("hm_roi_mean_u8", "hm_roi_mean_f64")
HOT = ("hm_hot_pixel_filter_u8", "hm_hot_pixel_filter_f64")


@contextlib.contextmanager
def on_device(*symbols):
    """Every one of `symbols` is called in the HIP library inside the block, none of them in the host library."""
    hip, host = nat.hip_lib.calls, nat.host_lib().calls
    before = {s: (hip[s], host[s]) for s in symbols}
    yield
    for s, (d, h) in before.items():
        assert hip[s] > d and host[s] == h, (s, hip[s] - d, host[s] - h)


@STD
@pytest.mark.parametrize("n", sl.HIST_COUNTS)
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_hist_counts(C_, n, use_std):
    with on_device("hm_channel_histogram", "hm_channel_minmax"):
        sl.check_hist_counts(DEV, C_, n, use_std)


@STD
@pytest.mark.parametrize("bins,C_", sl.HIST_BINS)
def test_hist_bins(bins, C_, use_std):
    with on_device(*HIST):
        sl.check_hist_bins(DEV, bins, C_, use_std)


def test_hist_above_limit():
    with on_device(*HIST):
        sl.check_hist_above_limit(DEV)


@STD
@pytest.mark.parametrize("lo,hi,bins,C_,differ", sl.EDGE_SETS)
def test_hist_edges(lo, hi, bins, C_, differ, use_std):
    with on_device(*HIST):
        sl.check_hist_edges(DEV, lo, hi, bins, C_, use_std)


@STD
def test_hist_subsets(use_std):
    with on_device("hm_channel_histogram", "hm_channel_minmax"):
        sl.check_hist_subsets(DEV, use_std)


@STD
def test_hist_unmasked(use_std):
    with on_device(*HIST):
        sl.check_hist_unmasked(DEV, use_std)


@STD
def test_hist_nothing_to_count(use_std):
    with on_device("hm_channel_histogram", "hm_channel_minmax"):
        sl.check_hist_nothing_to_count(DEV, use_std)


@STD
def test_hist_constant(use_std):
    with on_device("hm_channel_histogram", "hm_channel_minmax"):
        sl.check_hist_constant(DEV, use_std)


def test_hist_special_stds():
    with on_device(*HIST):
        sl.check_hist_special_stds(DEV)


@STD
def test_hist_nan_ends(use_std):
    with on_device("hm_channel_histogram", "hm_channel_minmax"):
        sl.check_hist_nan_ends(DEV, use_std)


@STD
def test_hist_offset_view(use_std):
    with on_device("hm_channel_histogram", "hm_channel_minmax"):
        sl.check_hist_offset_view(DEV, use_std)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_roi_small(C_, f64):
    with on_device(ROI[f64]):
        sl.check_roi_small(DEV, C_, f64)


@pytest.mark.parametrize("f64", [False, True])
def test_roi_large(f64):
    with on_device(ROI[f64]):
        sl.check_roi_large(DEV, f64)


def test_roi_offset_view():
    with on_device(ROI[1]):
        sl.check_roi_offset_view(DEV)


def test_roi_status():
    with on_device(*ROI):
        sl.check_roi_status(DEV)


@pytest.mark.parametrize("C_", [1, 2, 4])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_hot_spans(k, C_):
    with on_device(*HOT):
        sl.check_hot_spans(DEV, k, C_)


@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("shape", sl.THIN_SHAPES)
def test_hot_thin(shape, k):
    with on_device(*HOT):
        sl.check_hot_thin(DEV, shape, k)


def test_hot_thresholds():
    with on_device(*HOT):
        sl.check_hot_thresholds(DEV)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_hot_ties(k):
    with on_device(*HOT):
        sl.check_hot_ties(DEV, k)


def test_hot_unaligned_k7():
    with on_device(HOT[0]):
        sl.check_hot_unaligned_k7(DEV)
