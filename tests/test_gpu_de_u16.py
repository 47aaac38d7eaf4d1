"""The differential-evolution generation step for 9- to 16-bit cameras on the MI355X (hm_de_u16.hip through engine.DEPlanU16,
solve_channel_u16 and calibration_u16): the checks of tests/test_de_u16_host.py on device stacks, plus what only exists on the device:
graph replay against eager launches, bit for bit, the placements of the candidate's row, the device build against the host build, and the
host build never being reached."""
import numpy as np
import pytest

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from camera_linearity_amd import icrf_calibration as ic

import test_de_u16_host as du

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("b,S,P", du.GENERATION_CASES)
def test_one_generation_matches_restatement(b, S, P):
    calls = nat.hip_lib.calls["hm_de_generation_u16"]
    du.check_one_generation(DEV, b, S, P)
    assert nat.hip_lib.calls["hm_de_generation_u16"] == calls + 6


@pytest.mark.parametrize("b", [9, 10])
def test_row_walk_borders(b):
    du.check_row_walk_borders(DEV, b)


@pytest.mark.parametrize("b", [13, 14, 16])
def test_row_walk_borders_across_trips_and_slabs(b):
    """From 11 bits on the walk takes trips of eight segments (2048 DNs), from 14 bits on the trips are dealt to slabs of one (14 bits) or
    two (16 bits) trips, one workgroup each: ties at a trip's and a slab's first DN (the neighbour is the carried value, or the row the slab
    recomputes), one DN to either side, inside a later trip and at the row's end - every one must reach the member's one verdict byte."""
    pr = du.make_problem(DEV, b, P=1)
    n = pr["n"]
    pca, pop, straight = np.zeros((n, 1)), np.random.default_rng(13).random((8, 1)), np.linspace(0, 1, n)
    for d in (None, 2047, 2048, 2049, 4096, 4097, 6144, 6400, n - 2048, n - 1):
        mean = straight.copy()
        if d == n - 1:
            mean[d - 1] = mean[d]
        elif d is not None:
            mean[d] = mean[d - 1]
        plan = du.make_plan(pr, pop, mean=mean, pca=pca)
        plan.launch()
        np.testing.assert_array_equal(du.host(plan.icrf), np.tile(mean, (8, 1)))
        assert np.all(du.host(plan.valid) == (d is None)), d


def test_same_trial_as_the_8_bit_entry():
    du.check_same_trial_as_8_bit(DEV)


def test_determinism_check_every_variants_and_graph_replay():
    first = du.check_determinism(DEV)                                     # graph replay, check_every 1, 2, 3 and 8, variants 0, 1, 2
    pr = du.make_problem(DEV, 12)
    for ce in (1, 8):
        assert du.same(du.solve_state(pr, 7, ce, graph=False), first), ce    # the same calls launched eagerly
    assert engine.energy_kernel(24 * 24, 5, 32, False, 12, 1) != engine.energy_kernel(24 * 24, 5, 32, False, 12, 2)


def test_std_stack_passes_through():
    """A std stack takes the energy entry's weighted kernels: the generation step hands it on unchanged."""
    import torch
    pr = du.make_problem(DEV, 12)
    rng = np.random.default_rng(2)
    sd = torch.as_tensor(0.004 * (1 + rng.random(du.SHAPE)), device=DEV)
    pop = du.near_optimum(pr, rng, 16, 0.1)
    plan = engine.DEPlanU16(pr["stack"], sd, pr["t"], pr["mean"], pr["pca"], -1.0, 1.0, pop, pr["lower"], pr["upper"], 3, 100, bit_depth=12)
    plan.launch()
    plan.launch()
    valid = du.host(plan.valid).astype(bool)
    ref = engine.linearity_energy(pr["stack"], sd, pr["t"], plan.icrf, pr["lower"], pr["upper"], valid, True, bit_depth=12).cpu().numpy()
    np.testing.assert_array_equal(du.host(plan.trial_energies), ref)
    assert valid.any()


def test_stopping_and_frozen_state():
    du.check_stopping(DEV)


def test_end_to_end():
    du.check_end_to_end(DEV)


def test_plan_refusals():
    du.check_plan_refusals(DEV)


def test_device_stack_never_reaches_the_host_build():
    pr = du.make_problem(DEV, 10)
    assert pr["stack"].is_cuda
    hip, h = nat.hip_lib.calls, nat.host_lib().calls
    before = (h["hm_de_generation_u16"], h["hm_linearity_energy_u16"], hip["hm_de_generation_u16"], hip["hm_de_generation"])
    icrf, e, n_it = ic.solve_channel_u16(pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0, 10, seed=7, max_iterations=2)
    assert (h["hm_de_generation_u16"], h["hm_linearity_energy_u16"]) == before[:2]
    assert hip["hm_de_generation_u16"] > before[2] and hip["hm_de_generation"] == before[3] and n_it == 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):             # a host stack handed to the HIP backend is an error, not a fallback
        engine.DEPlanU16(pr["stack"].cpu(), None, pr["t"], pr["mean"], pr["pca"], -1.0, 1.0, np.full((8, 3), 0.5), 20, 1000, 1, 10, bit_depth=10)


@pytest.mark.parametrize("b", [10, 16])
def test_device_and_host_builds_agree(b):
    """The two builds of the ABI run the same algorithm: the same accepted / rejected pattern over ten generations, energies to 1e-10
    (the criterion of tests/test_gpu_de.py::test_device_and_host_builds_agree)."""
    out = []
    for dev in (DEV, "cpu"):
        pr = du.make_problem(dev, b)
        rng = np.random.default_rng(6)
        pop = rng.random((32, 3))
        pop[:16] = du.near_optimum(pr, rng, 16, 0.2)
        plan = du.make_plan(pr, pop, seed=9, max_generations=10, tol=0.0)
        plan.run(4)
        out.append((du.host(plan.population), du.host(plan.energies)))
    fin = np.isfinite(out[0][1])
    np.testing.assert_array_equal(fin, np.isfinite(out[1][1]))
    np.testing.assert_allclose(out[0][1][fin], out[1][1][fin], rtol=1e-10)
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=1e-10)
