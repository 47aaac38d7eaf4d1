"""The differential-evolution generation step on the MI355X (hm_de.hip through engine.DEPlan and solve_channel(solver="device")): the
checks of tests/test_de_host.py - the NumPy restatement of the algorithm lives there - on device stacks, plus what only exists on the
device: graph replay against eager launches, bit for bit, and the host build never being reached."""
import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import icrf_calibration as ic

import test_de_host as de

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPE = (40, 40, 6)              # the stack of test_calibration_recovers_response


@pytest.mark.parametrize("S,P", [(8, 1), (8, 3), (64, 3), (64, 5), (128, 1), (128, 5)])
def test_one_generation_matches_restatement(S, P):
    calls = nat.hip_lib.calls["hm_de_generation"]
    de.check_one_generation(DEV, S, P, SHAPE)
    assert nat.hip_lib.calls["hm_de_generation"] == calls + 6


def test_best_index_ties_go_to_the_lowest_index():
    de.check_ties(DEV, SHAPE)


def test_twenty_generations_follow_the_restatement():
    de.check_many_generations(DEV, SHAPE)


def test_determinism_check_every_and_graph_replay():
    p, e, t, st = de.check_determinism(DEV, SHAPE)                       # graph replay, check_every 1, 2, 3 and 8
    pr = de.make_problem(DEV, *SHAPE)
    for ce in (1, 8):
        p2, e2, t2, st2 = de.solve_state(pr, 7, ce, graph=False)         # the same calls launched eagerly
        assert p2.tobytes() == p.tobytes() and e2.tobytes() == e.tobytes() and t2.tobytes() == t.tobytes() and st2 == st, ce


def test_pair_major_energy_path_and_std_stack():
    """More than eight frames take the energy launcher's pair-major kernels, and a std stack its weighted variant: the generation step
    passes both through unchanged."""
    rng = np.random.default_rng(2)
    X, Y, N = 16, 16, 10
    dn = torch.as_tensor(np.sort(rng.integers(0, 256, (X, Y, N)).astype(np.uint8), axis=2), device=DEV)
    sd = torch.as_tensor(0.004 * (1 + rng.random((X, Y, N))), device=DEV)
    pr = de.make_problem(DEV, *SHAPE)
    pr = dict(pr, stack=dn, t=1e-3 * 2.0 ** np.arange(N))
    pop = 0.5 * (pr["true"] + 1) + 0.1 * (rng.random((16, 3)) - 0.5)
    from camera_linearity_amd import engine
    plan = engine.DEPlan(dn, sd, pr["t"], pr["mean"], pr["pca"], -1.0, 1.0, pop, 5, 250, 3, 100)
    plan.launch()
    plan.launch()
    valid = de.host(plan.valid).astype(bool)
    ref = engine.linearity_energy(dn, sd, pr["t"], plan.icrf, 5, 250, valid, True).cpu().numpy()
    np.testing.assert_array_equal(de.host(plan.trial_energies), ref)
    assert valid.any()


def test_stopping():
    de.check_stopping(DEV, SHAPE)


def test_end_to_end():
    de.check_end_to_end(DEV, SHAPE)


def test_device_stack_never_reaches_the_host_build():
    pr = de.make_problem(DEV, *SHAPE)
    assert pr["stack"].is_cuda
    hip, h = nat.hip_lib.calls, nat.host_lib().calls
    before = (h["hm_de_generation"], h["hm_linearity_energy"], hip["hm_de_generation"])
    icrf, e, n_it = ic.solve_channel(pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0, seed=7, max_iterations=2, solver="device")
    assert (h["hm_de_generation"], h["hm_linearity_energy"]) == before[:2]
    assert hip["hm_de_generation"] > before[2] and n_it == 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):             # a host stack handed to the HIP backend is an error, not a fallback
        from camera_linearity_amd import engine
        engine.DEPlan(pr["stack"].cpu(), None, pr["t"], pr["mean"], pr["pca"], -1.0, 1.0, np.full((8, 3), 0.5), 5, 250, 1, 10)


def test_device_and_host_builds_agree():
    """The two builds of the ABI run the same algorithm: the same accepted / rejected pattern over ten generations, energies to 1e-10."""
    out = []
    for dev in (DEV, "cpu"):
        pr = de.make_problem(dev, *SHAPE)
        rng = np.random.default_rng(6)
        pop = rng.random((32, 3))
        pop[:16] = 0.5 * (pr["true"] + 1) + 0.2 * (rng.random((16, 3)) - 0.5)
        plan = de.make_plan(pr, pop, seed=9, max_generations=10, tol=0.0)
        plan.run(4)
        out.append((de.host(plan.population), de.host(plan.energies)))
    fin = np.isfinite(out[0][1])
    np.testing.assert_array_equal(fin, np.isfinite(out[1][1]))
    np.testing.assert_allclose(out[0][1][fin], out[1][1][fin], rtol=1e-10)
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=1e-10)
