"""The kernel density estimate (csrc/hm_kde.hip) on the MI355X at the limits of its ABI: the checks of tests/test_kde_limits_host.py - the
long-double references, the derived bounds and every case live there - on device memory through the raw C ABI, and the errors of the
Python path (tests/test_kde_host.py's check functions) on a HipMeasurand. Every test asserts that the device symbol ran and the host one
did not."""
import contextlib

import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import kde
from camera_linearity_amd.measurand import HipMeasurand

import test_kde_host as kh
import test_kde_limits_host as kl
from test_kde_limits_host import report_observed_maxima  # noqa: F401  (prints the observed maxima after this module too)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EVAL, MOM = "hm_kde_evaluate", "hm_kde_moments"


@contextlib.contextmanager
def on_device(*symbols):
    """Every one of `symbols` is called in the HIP library inside the block, none of them in the host library."""
    hip, host = nat.hip_lib.calls, nat.host_lib().calls
    before = {s: (hip[s], host[s]) for s in symbols}
    yield
    for s, (d, h) in before.items():
        assert hip[s] > d and host[s] == h, (s, hip[s] - d, host[s] - h)


def dev_run(x, s=None, *a, **k):
    up = lambda v: None if v is None else torch.as_tensor(v, device=DEV)  # noqa: E731
    return kde.kernel_density_estimate(HipMeasurand(up(x), up(s)), *a, **k)


@pytest.mark.parametrize("kind", kl.STD_KINDS)
@pytest.mark.parametrize("C_", kl.MOMENT_CHANNELS)
@pytest.mark.parametrize("n", kl.MOMENT_COUNTS)
def test_moments(n, C_, kind):
    with on_device(MOM):
        kl.check_moments(DEV, n, C_, kind)


@pytest.mark.parametrize("n", kl.COUNTS)
def test_element_counts(n):
    with on_device(EVAL):
        kl.check_estimate(DEV, "count", n)


@pytest.mark.parametrize("m", kl.GRID_SIZES)
def test_grid_sizes(m):
    with on_device(EVAL):
        kl.check_estimate(DEV, "grid", m)


@pytest.mark.parametrize("k", kl.SUM_CHUNKS)
def test_chunk_counts(k):
    with on_device(EVAL):
        kl.check_estimate(DEV, "sum", k)


def test_far_tail():
    with on_device(EVAL):
        kl.check_far_tail(DEV)


def test_overflowing_quotient():
    with on_device(EVAL):
        kl.check_overflow(DEV)


def test_workspace_size():
    with on_device(EVAL, MOM):
        kl.check_workspace_size(DEV)


def test_errors_match_reference():
    with on_device(MOM):
        kh.check_errors_match_reference(dev_run)


def test_inf_std_counts_with_weight_zero():
    with on_device(EVAL, MOM):
        kh.check_inf_std_counts_with_weight_zero(dev_run)


def test_all_negative_weights():
    with on_device(EVAL, MOM):
        kh.check_all_negative_weights(dev_run)
