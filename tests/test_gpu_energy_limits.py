"""The energy kernels (csrc/hm_energy.hip: k_energy_pixel<N, STD> for every N, k_energy_partial up to HM_MAX_FRAMES, k_energy_final)
and the generation step (csrc/hm_de.hip: k_de_select's padded tree, the batch kernels at HM_DE_MAX_PROBLEMS) on the MI355X at the limits
of their ABI: the checks of tests/test_energy_limits_host.py - the extended-precision reference, the derived bound and every case
live there - on device stacks. The reference of a case is computed once per session and shared with the host checks."""
import numpy as np
import pytest

from camera_linearity_amd import _native as nat

import test_energy_limits_host as el
from test_energy_limits_host import report_observed_maxima  # noqa: F401  (prints the observed maxima after this module too)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("name", list(el.CASES))
def test_energy_case(name):
    hip, h = nat.hip_lib.calls, nat.host_lib().calls
    before = (hip["hm_linearity_energy"], h["hm_linearity_energy"])
    el.check_energy_case(DEV, name)
    assert hip["hm_linearity_energy"] == before[0] + len(el.case(name)["modes"]) and h["hm_linearity_energy"] == before[1]


def test_both_geometries_within_their_bounds_of_one_reference():
    el.check_both_geometries(DEV)


@pytest.mark.parametrize("S,P", el.DE_CASES)
def test_generation_at_limits(S, P):
    calls = nat.hip_lib.calls["hm_de_generation"]
    el.check_generation_at_limits(DEV, S, P)
    assert nat.hip_lib.calls["hm_de_generation"] == calls + 4


def test_ties_above_256():
    el.check_ties_above_256(DEV)


def test_batch_of_64():
    el.check_batch_of_64(DEV)


def test_batch_of_3_with_45():
    el.check_batch_of_3_with_45(DEV)
