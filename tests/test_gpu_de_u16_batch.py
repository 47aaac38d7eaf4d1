"""K differential-evolution problems per call for 9- to 16-bit cameras on the MI355X (the batched kernels of hm_de_u16.hip and
hm_energy_u16.hip through engine.DEBatchPlanU16, solve_channel_u16(batched=True), calibration_u16(batched=True)): the checks of
tests/test_de_u16_batch_host.py on device stacks - a batch against K single plans, bytes of every state array and status word - plus what
only exists on the device: graph replay against eager launches, the two builds side by side, and the host build never being reached."""
import numpy as np
import pytest

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine

import test_de_u16_batch_host as db
from test_de_host import host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("b,S,P", db.EQUAL_CASES)
def test_batch_equals_singles(b, S, P):
    calls = (nat.hip_lib.calls["hm_de_generation_u16_batch"], nat.hip_lib.calls["hm_de_generation_u16"])
    db.check_batch_equals_singles(DEV, b, S, P)
    assert nat.hip_lib.calls["hm_de_generation_u16_batch"] == calls[0] + 13              # one call per generation for the three problems
    assert nat.hip_lib.calls["hm_de_generation_u16"] == calls[1] + 3 * 13                # (the single plans it is compared with)


def test_geometry_rule_is_per_problem():
    db.check_geometry_is_per_problem(DEV)


@pytest.mark.parametrize("b", [12, 16])
def test_pair_major_and_std(b):
    db.check_pair_major_and_std(DEV, b)


def test_shared_stacks():
    db.check_shared_stacks(DEV)


@pytest.mark.parametrize("b", [12, 14])
def test_problems_stop_at_different_times(b):
    db.check_problems_stop_at_different_times(DEV, b)


@pytest.mark.parametrize("b", [12, 14])
def test_stopped_problem_is_frozen_while_others_run(b):
    db.check_frozen_among_running(DEV, b)


def test_determinism_check_every_graph_replay_and_variants():
    db.check_determinism(DEV, graphs=(True, False))                                      # graph replay and the same calls launched eagerly


def test_plan_refusals():
    db.check_plan_refusals(DEV)


def test_calibration_batched_equals_sequential():
    db.check_calibration_batched(DEV, nat.hip_lib)


def test_restarts_batched_equal_the_sequential_restarts():
    db.check_restarts(DEV)


@pytest.mark.parametrize("b", [10, 16])
def test_device_and_host_builds_agree(b):
    """The two builds of the ABI run the same algorithm on a K = 3 batch: the same finite pattern over ten generations, energies to 1e-10,
    populations to 1e-10 (the bounds of test_gpu_de_batch.py::test_device_and_host_builds_agree)."""
    out = []
    for dev in (DEV, "cpu"):
        q = db.make_batch(dev, b, 3, (40, 40, 6), 32, 3, seeds=(9, 10, 11), max_generations=10)
        plan = db.batch_plan(q)
        sts = plan.run(4)
        assert all(st["generation"] == 10 for st in sts)
        out.append((host(plan.population), host(plan.energies)))
    fin = np.isfinite(out[0][1])
    assert fin.any(axis=1).all()
    np.testing.assert_array_equal(fin, np.isfinite(out[1][1]))
    np.testing.assert_allclose(out[0][1][fin], out[1][1][fin], rtol=1e-10)
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=1e-10)


def test_device_batch_never_reaches_the_host_build():
    q = db.make_batch(DEV, 10, 2, (40, 40, 6), 8, 3, seeds=(1, 2), max_generations=4)
    assert all(s.is_cuda for s in q["stacks"])
    hip, h = nat.hip_lib.calls, nat.host_lib().calls
    before = (h["hm_de_generation_u16_batch"], h["hm_de_generation_u16"], h["hm_linearity_energy_u16"], hip["hm_de_generation_u16_batch"])
    sts = db.batch_plan(q).run(2)
    assert (h["hm_de_generation_u16_batch"], h["hm_de_generation_u16"], h["hm_linearity_energy_u16"]) == before[:3]
    assert hip["hm_de_generation_u16_batch"] > before[3] and all(st["generation"] == 4 for st in sts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                           # host stacks handed to the HIP backend are an error, not a fallback
        engine.DEBatchPlanU16([s.cpu() for s in q["stacks"]], None, q["t"], q["means"], q["pcas"], -1.0, 1.0, q["pop"], 20, 1000, q["seeds"], 10,
                              bit_depth=10)
