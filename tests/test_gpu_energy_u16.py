"""The ICRF-calibration energy on uint16 DN stacks (csrc/hm_energy_u16.hip: k_energy_pixel_u16<N, STD, LUT>, k_energy_partial_u16<STD, LUT>,
the candidate's row in LDS or gathered from global memory) on the MI355X: the checks of tests/test_energy_u16_host.py - the embedding, the
oracle comparison, the bounds and every case live there - on device stacks."""
import pytest

from camera_linearity_amd import _native as nat

import test_energy_u16_host as eu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("depth", eu.EMBED_DEPTHS)
@pytest.mark.parametrize("shape", eu.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_embedding_bit_patterns(shape, depth):
    hip, h = nat.hip_lib.calls, nat.host_lib().calls
    before = (hip["hm_linearity_energy_u16"], h["hm_linearity_energy_u16"])
    eu.check_embedding(DEV, shape, depth)
    assert hip["hm_linearity_energy_u16"] == before[0] + len(eu.MODES) * len(eu.variants(depth)) and h["hm_linearity_energy_u16"] == before[1]


@pytest.mark.parametrize("with_std", [False, True])
@pytest.mark.parametrize("depth", eu.ORACLE_DEPTHS)
@pytest.mark.parametrize("shape", eu.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_oracle(shape, depth, with_std):
    eu.check_oracle(DEV, shape, depth, with_std)


@pytest.mark.parametrize("depth", [9, 12, 15])
def test_stray_high_bits_are_masked(depth):
    eu.check_stray_high_bits(DEV, depth)


@pytest.mark.parametrize("name", list(eu.EDGE_CHECKS))
def test_edges(name):
    eu.EDGE_CHECKS[name](DEV)


def test_variant_1_at_15_bits_is_not_implemented():
    import numpy as np
    import torch
    dn = torch.zeros((3, 3, 2), dtype=torch.uint16, device=DEV)
    with pytest.raises(NotImplementedError):
        eu.eng(DEV).linearity_energy(dn, None, [1.0, 2.0], np.linspace(0, 1, 2 ** 15)[None], 5, 2 ** 15 - 6, bit_depth=15, variant=1)


def test_python_surface():
    eu.check_python_surface(DEV)


def test_calibration_at_12_bits():
    calls = nat.hip_lib.calls["hm_linearity_energy_u16"]
    eu.check_calibration_12_bits(DEV)
    assert nat.hip_lib.calls["hm_linearity_energy_u16"] > calls + 40
