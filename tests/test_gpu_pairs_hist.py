"""The all-pairs linearity distributions (csrc/hm_stats_hist.hip: k_pairs_hist, k_pairs_minmax, k_pairs_minmax_final) on the MI355X: the
checks of tests/test_pairs_hist_host.py - the reference, the derived bound and every case live there - on device tensors. Every test
asserts that the device symbols ran and the host ones did not."""
import pytest

from camera_linearity_amd import _native as nat

import test_pairs_hist_host as ph
from test_gpu_stats_limits import on_device
from test_stats_limits_host import report_observed_maxima  # noqa: F401  (prints the observed maxima after this module too)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STD = pytest.mark.parametrize("use_std", [False, True])
BOTH = ("hm_pairs_histogram", "hm_pairs_minmax")


@STD
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
@pytest.mark.parametrize("name,npix", ph.SIZES)
def test_sizes(name, npix, C_, use_std):
    with on_device(*BOTH):
        ph.check_sizes(DEV, npix, C_, use_std)


@STD
def test_masks(use_std):
    with on_device(*BOTH):
        ph.check_masks(DEV, use_std)


@STD
def test_seven_frames(use_std):
    with on_device(*BOTH):
        ph.check_seven_frames(DEV, use_std)


@STD
def test_thirty_two_frames(use_std):
    with on_device(*BOTH):
        ph.check_thirty_two_frames(DEV, use_std)


@STD
@pytest.mark.parametrize("bins,C_", ph.BINS)
def test_bins(bins, C_, use_std):
    with on_device(*BOTH):
        ph.check_bins(DEV, bins, C_, use_std)


def test_above_limit():
    with on_device("hm_pairs_histogram"):
        ph.check_above_limit(DEV)


@STD
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("lo,hi,bins,C_", ph.EDGE_SETS)
def test_edges(lo, hi, bins, C_, kind, use_std):
    with on_device(*BOTH):
        ph.check_edges(DEV, lo, hi, bins, C_, kind, use_std)


def test_specials():
    with on_device(*BOTH):
        ph.check_specials(DEV)


@STD
def test_thresholds(use_std):
    with on_device(*BOTH):
        ph.check_thresholds(DEV, use_std)


@STD
def test_constant(use_std):
    with on_device(*BOTH):
        ph.check_constant(DEV, use_std)


@STD
def test_alignment(use_std):
    with on_device(*BOTH):
        ph.check_alignment(DEV, use_std)


def test_status_codes():
    """The table of bad calls gives the same codes on the HIP build as on the host build."""
    with on_device(*BOTH):
        device_codes = ph.status_table(DEV)
    assert device_codes == ph.status_table("cpu")


def test_series():
    with on_device(*BOTH):
        ph.check_series(DEV, lambda: nat.hip_lib.calls["hm_pairs_histogram"])
