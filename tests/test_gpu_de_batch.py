"""K differential-evolution problems per call on the MI355X (hm_de.hip / hm_energy.hip batched kernels through engine.DEBatchPlan,
solve_channel(restarts=...), calibration(batched=True)): the checks of tests/test_de_batch_host.py on device stacks - a batch against K
single plans, bytes of every state array and status word - plus what only exists on the device: graph replay against eager launches, the
two builds side by side, and the host build never being reached."""
import numpy as np
import pytest

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine

import test_de_batch_host as db
from test_de_host import host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("S,P", [(8, 3), (16, 5)])
def test_batch_equals_singles(S, P):
    calls = (nat.hip_lib.calls["hm_de_generation_batch"], nat.hip_lib.calls["hm_de_generation"])
    db.check_batch_equals_singles(DEV, S, P)
    assert nat.hip_lib.calls["hm_de_generation_batch"] == calls[0] + 13                  # one call per generation for the three problems
    assert nat.hip_lib.calls["hm_de_generation"] == calls[1] + 3 * 13                    # (the single plans it is compared with)


def test_geometry_rule_is_per_problem():
    db.check_geometry_is_per_problem(DEV)


def test_pair_major_and_std():
    db.check_pair_major_and_std(DEV)


def test_shared_stacks():
    db.check_shared_stacks(DEV)


def test_problems_stop_at_different_times():
    db.check_problems_stop_at_different_times(DEV)


def test_determinism_check_every_and_graph_replay():
    db.check_determinism(DEV, graphs=(True, False))                                      # graph replay and the same calls launched eagerly


def test_calibration_batched_equals_sequential():
    db.check_calibration_batched(DEV, nat.hip_lib)


def test_restarts_return_the_best_of_the_single_solves():
    db.check_restarts(DEV)


def test_device_and_host_builds_agree():
    """The two builds of the ABI run the same algorithm on a K = 3 batch: the same finite pattern over ten generations, energies to 1e-10,
    populations to 1e-10 (the bounds of test_gpu_de.py::test_device_and_host_builds_agree)."""
    out = []
    for dev in (DEV, "cpu"):
        b = db.make_batch(dev, 3, (40, 40, 6), 32, 3, seeds=(9, 10, 11), max_generations=10)
        plan = db.batch_plan(b)
        sts = plan.run(4)
        assert all(st["generation"] == 10 for st in sts)
        out.append((host(plan.population), host(plan.energies)))
    fin = np.isfinite(out[0][1])
    assert fin.any(axis=1).all()
    np.testing.assert_array_equal(fin, np.isfinite(out[1][1]))
    np.testing.assert_allclose(out[0][1][fin], out[1][1][fin], rtol=1e-10)
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=1e-10)


def test_device_batch_never_reaches_the_host_build():
    b = db.make_batch(DEV, 2, (40, 40, 6), 8, 3, seeds=(1, 2), max_generations=4)
    assert all(s.is_cuda for s in b["stacks"])
    hip, h = nat.hip_lib.calls, nat.host_lib().calls
    before = (h["hm_de_generation_batch"], h["hm_de_generation"], h["hm_linearity_energy"], hip["hm_de_generation_batch"])
    sts = db.batch_plan(b).run(2)
    assert (h["hm_de_generation_batch"], h["hm_de_generation"], h["hm_linearity_energy"]) == before[:3]
    assert hip["hm_de_generation_batch"] > before[3] and all(st["generation"] == 4 for st in sts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                           # host stacks handed to the HIP backend are an error, not a fallback
        engine.DEBatchPlan([s.cpu() for s in b["stacks"]], None, b["t"], b["means"], b["pcas"], -1.0, 1.0, b["pop"], 5, 250, b["seeds"], 10)
