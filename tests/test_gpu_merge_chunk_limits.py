"""The chunked merge (csrc/hm_merge_chunk.hip) on the MI355X at the limits of its ABI: the checks of tests/test_merge_chunk_limits_host.py -
the cases, the two criteria and the predicted kernel names live there - on device tensors. Every test asserts that hm_merge ran in the
HIP library (the checks themselves assert `plan.kernels`, i.e. that the launches were merge_chunk<...> with the predicted vec and hot)."""
import contextlib

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine

import test_merge_chunk_limits_host as mc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = pytest.mark.parametrize("f64", [False, True], ids=["u8", "f64"])


@contextlib.contextmanager
def on_device(host_too=False):
    """hm_merge is called in the HIP library inside the block, and (unless the check compares with the host build) not in the host library."""
    hip = nat.hip_lib.calls
    host = nat.host_lib().calls
    before = hip["hm_merge"], host["hm_merge"]
    yield
    assert hip["hm_merge"] > before[0]
    assert host_too or host["hm_merge"] == before[1]


@F64
@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("n,chunk", mc.BOUNDARIES)
def test_boundaries(n, chunk, f64, mode):
    with on_device():
        mc.check_boundaries(DEV, n, chunk, f64, mode)


@F64
@pytest.mark.parametrize("mode", mc.MODES)
@pytest.mark.parametrize("n", mc.LONG)
def test_long_stacks(n, f64, mode):
    with on_device(host_too=not f64):
        mc.check_long(DEV, n, f64, mode)


@F64
@pytest.mark.parametrize("with_std", [False, True])
@pytest.mark.parametrize("chunk", [2, 3])
@pytest.mark.parametrize("c", [1, 2, 4])
def test_channels(c, chunk, with_std, f64):
    with on_device():
        mc.check_channels(DEV, c, chunk, with_std, f64)


@F64
@pytest.mark.parametrize("tile", mc.ROW_TILES)
def test_row_tiles(tile, f64):
    with on_device():
        mc.check_row_tile(DEV, tile, f64)


@F64
@pytest.mark.parametrize("mode,k", [("val", 3), ("std", 3), ("S", 3), ("std", 5), ("S", 5)])
def test_hot_placement(f64, mode, k):
    with on_device():
        mc.check_hot_placement(DEV, f64, mode, k)


@pytest.mark.parametrize("mode", ["val", "std"])
def test_grid_stride(mode):
    assert mc.stride_elems(DEV) > 2 * 8 * 256 * 2
    with on_device():
        mc.check_grid_stride(DEV, mode)


@F64
def test_sum_buffer(f64):
    with on_device():
        mc.check_sum_buffer(DEV, f64)


def test_uint16_frames_refuse_forced_chunking():
    """uint16 frames have no chunked path: NotImplementedError before any call into the library."""
    calls = sum(v for k, v in nat.hip_lib.calls.items() if k.startswith("hm_merge_u16") and not k.endswith("_bytes"))
    f16 = [torch.as_tensor(np.full((4, 6, 3), 100 * (i + 1), np.uint16), device=DEV) for i in range(3)]
    icrf = np.stack([np.linspace(0, 1, 4096)] * 3, axis=1)
    with pytest.raises(NotImplementedError):
        engine.plan_merge(f16, [1e-3, 2e-3, 4e-3], icrf, bit_depth=12, variant=-2)
    assert sum(v for k, v in nat.hip_lib.calls.items() if k.startswith("hm_merge_u16") and not k.endswith("_bytes")) == calls
