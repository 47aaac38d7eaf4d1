"""The Welford producer on uint16 frames (csrc/hm_welford_u16.hip: k_welford_u16<M2, PLACE> with the frame value from a table in LDS,
computed in the lane, or gathered from the ICRF in global memory; k_welford_finalize_u16) on the MI355X: the checks of
tests/test_welford_u16_host.py - the embedding, the oracle comparison, the exhaustive quotient, the range cases, alignment, finalize and
the Python surface live there with every shape - on device tensors."""
import pytest

from camera_linearity_amd import _native as nat

import test_welford_u16_host as wu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _calls():
    return nat.hip_lib.calls["hm_welford_update_u16"], nat.host_lib().calls["hm_welford_update_u16"]


@pytest.mark.parametrize("depth", wu.DEPTHS)
@pytest.mark.parametrize("shape", wu.SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_embedding_bit_patterns(shape, depth):
    hip, host = _calls()
    wu.check_embedding(DEV, shape, depth)
    launches = (1 + 2) * len(wu.variants(depth, shape[2], True)) + (3 * len(wu.variants(16, shape[2], False)) if depth == 16 else 0)
    assert _calls() == (hip + launches, host)                              # 9 frames: one launch, 45: two; all through the HIP library


@pytest.mark.parametrize("with_icrf", [False, True])
@pytest.mark.parametrize("depth", wu.DEPTHS)
@pytest.mark.parametrize("shape", wu.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_oracle(shape, depth, with_icrf):
    hip, host = _calls()
    wu.check_oracle(DEV, shape, depth, with_icrf)
    assert _calls()[0] > hip and _calls()[1] == host


@pytest.mark.parametrize("depth", [9, 12, 15])
def test_stray_high_bits_are_masked(depth):
    wu.check_stray_high_bits(DEV, depth)


@pytest.mark.parametrize("depth", range(9, 17))
def test_computed_quotient_is_the_ieee_quotient(depth):
    assert wu.kernel_of(2 ** depth, 1, 1, False, True, depth, wu.COMPUTED) == f"k_welford_u16<m2=1,tab=computed,bits={depth}>"
    wu.check_computed_quotient(DEV, depth)


@pytest.mark.parametrize("case", wu.RANGE_CASES)
def test_fast_division_range(case):
    wu.check_fast_division_range(DEV, case)


@pytest.mark.parametrize("with_icrf", [False, True])
@pytest.mark.parametrize("shape", [(7, 9, 3), (12, 20, 3), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_alignment_and_tails(shape, with_icrf):
    for depth in (12, 16):
        wu.check_alignment(DEV, shape, depth, with_icrf)


@pytest.mark.parametrize("depth", wu.DEPTHS)
def test_finalize(depth):
    before = nat.hip_lib.calls["hm_welford_finalize_u16"]
    wu.check_finalize(DEV, depth)
    assert nat.hip_lib.calls["hm_welford_finalize_u16"] == before + 3


def test_rounding_out_of_range():
    wu.check_rounding_out_of_range(DEV)


def test_python_surface():
    hip, host = _calls()
    wu.check_python(DEV)
    assert _calls()[0] > hip and _calls()[1] == host
