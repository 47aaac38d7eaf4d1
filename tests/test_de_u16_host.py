"""The differential-evolution generation step for 9- to 16-bit cameras (hm_de_generation_u16, engine.DEPlanU16, solve_channel_u16,
calibration_u16) on the HOST build, against the NumPy restatement of tests/test_de_host.py (np_trial, np_select, uniform: imported, not
restated) and icrf_calibration.candidate_icrfs for the rows. The checks are functions of a device name: tests/test_gpu_de_u16.py runs the
same ones on the MI355X. Every stack is 24 x 24 x 5.

The camera is test_de_host.make_problem's at depth b, but for its mean ICRF: 0.5 xs + 0.5 xs**2, not xs**2, whose first step at 16 bits
(2.3e-10) would leave no margin for the verdict comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from camera_linearity_amd import icrf_calibration as ic

import test_de_host as de
from test_de_host import np_select, np_trial, uniform  # noqa: F401  (uniform: np_trial's draws)

SHAPE = (24, 24, 5)
F_LO, F_HI, CR, TOL = de.F_LO, de.F_HI, de.CR, de.TOL
host = de.host
poke = de.poke


def eng(dev):
    """engine on a device stack, the host build of the same functions on a host stack"""
    return engine if torch.device(dev).type == "cuda" else ic._engine_for(torch.zeros(1))


# ------------------------------------------------------------------------------------------------ the problem
_PROBLEMS = {}


def make_problem(device, b, P=3, channels=1):
    """make_problem's synthetic camera at depth b (computed once per (device, b, P, channels) and never changed)."""
    key = (str(device), b, P, channels)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    X, Y, N = SHAPE
    n = 2 ** b
    rng = np.random.default_rng(21)
    t = 1e-3 * 2.0 ** np.arange(N)
    xs = np.linspace(0, 1, n)
    pca = np.stack([np.sin(np.pi * (m + 1) * xs) / (m + 1) for m in range(P)], axis=1) * 0.1
    mean_icrf = 0.5 * xs + 0.5 * xs ** 2
    true_params = np.array([0.6, -0.3, 0.2, 0.1, -0.1][:P])
    true_icrf, ok = ic.candidate_icrfs(true_params, mean_icrf, pca)
    assert ok[0]
    rad = rng.random((X, Y)) * 2.5 / t[-1]
    lin = np.clip(rad[..., None] * t, 0, 1)
    dn = np.clip(np.around(np.interp(lin, true_icrf[0], xs) * (n - 1)), 0, n - 1).astype(np.uint16)
    frames = [dn[:, :, None, i].repeat(channels, 2) for i in range(N)]
    stacks, stds, tt = ic.initialize_channel_image_stacks(frames, t, None, 1, device=device, bit_depth=b)
    pr = dict(stacks=stacks, stack=stacks[0], t=tt, pca=pca, mean=mean_icrf, true=true_params, P=P, device=device, b=b, n=n,
              lower=5 << (b - 8), upper=250 << (b - 8), frames=frames)
    _PROBLEMS[key] = pr
    return pr


def make_plan(pr, pop, seed=11, max_generations=1 << 40, tol=TOL, energy_limit=0.0, variant=0, mean=None, pca=None):
    return eng(pr["device"]).DEPlanU16(pr["stack"], None, pr["t"], pr["mean"] if mean is None else mean, pr["pca"] if pca is None else pca,
                                       -1.0, 1.0, pop, pr["lower"], pr["upper"], seed, max_generations, (F_LO, F_HI), CR, tol, energy_limit,
                                       pr["b"], variant)


def energies_of(pr, icrfs, valid):
    return eng(pr["device"]).linearity_energy(pr["stack"], None, pr["t"], icrfs, pr["lower"], pr["upper"], valid, True, bit_depth=pr["b"])


def near_optimum(pr, rng, n, spread):
    return 0.5 * (pr["true"] + 1) + spread * (rng.random((n, pr["P"])) - 0.5)


# ------------------------------------------------------------------------------------------------ 1: one generation
MARGIN = 1e-11                # 100 x the row tolerance: a restated row within it of a verdict's boundary would make the comparison a coin toss


def clear_verdicts(icrfs):
    """-> (clearly valid, clearly invalid) per restated row, with MARGIN."""
    steps, inner = np.diff(icrfs, axis=1), icrfs[:, 1:-1]
    ok = np.all(steps > MARGIN, axis=1) & np.all(inner > MARGIN, axis=1) & np.all(inner < 1 - MARGIN, axis=1)
    bad = np.any(steps < -MARGIN, axis=1) | np.any(icrfs < -MARGIN, axis=1) | np.any(icrfs > 1 + MARGIN, axis=1)
    return ok, bad


def check_one_generation(device, b, S, P):
    pr = make_problem(device, b, P=P)
    n = pr["n"]
    rng = np.random.default_rng(100 * S + P)
    pop0 = rng.random((S, P))
    pop0[: S // 2] = near_optimum(pr, rng, S // 2, 0.1)                                  # half of the members near the optimum: valid rows
    plan = make_plan(pr, pop0, seed=1234 + S)
    assert tuple(plan.icrf.shape) == (S, n)
    plan.launch()                                                                        # generation 0: evaluates the population
    st = plan.read_status()
    assert st["generation"] == 0 and st["evaluations"] == S and st["stop"] == 0
    np.testing.assert_array_equal(host(plan.population), pop0)
    np.testing.assert_array_equal(host(plan.trial), pop0)                                # no draws
    E0 = host(plan.energies)
    assert np.isfinite(E0).sum() >= S // 4 and st["best_index"] == int(np.argmin(E0))
    n_replaced = n_invalid = 0
    for g in (1, 2, 7, 1000, 123456):
        poke(plan, nat.HM_DE_GENERATION, g)
        poke(plan, nat.HM_DE_STOP, 0)
        pop, E, best = host(plan.population), host(plan.energies), plan.read_status()["best_index"]
        assert best == int(np.argmin(E))
        ref = np_trial(pop, best, g, 1234 + S)
        m = ref["mutant"][ref["taken"]]
        assert np.all(np.minimum(np.abs(m), np.abs(m - 1)) > 1e-12)                      # no mutant component at the edge of [0, 1]
        plan.launch()
        trial = host(plan.trial)
        keep = ~ref["taken"]
        np.testing.assert_array_equal(trial[keep], pop[keep])                            # crossover mask and fill point: exact
        assert ref["taken"].any(axis=1).all()
        np.testing.assert_array_equal(trial[ref["replaced"]], ref["redraw"][ref["replaced"]])   # out-of-range replacements: exact draws
        np.testing.assert_allclose(trial, ref["trial"], rtol=0, atol=1e-14)
        n_replaced += int(ref["replaced"].sum())
        # candidate ICRFs and verdicts of the DEVICE's trial rows
        icrfs, valid = ic.candidate_icrfs(-1.0 + trial * 2.0, pr["mean"], pr["pca"])
        assert icrfs.shape == (S, n) and np.all(icrfs[:, -1] == 1.0) and np.all(icrfs[:, 0] == 0.0)
        ok, bad = clear_verdicts(icrfs)
        assert np.all(ok ^ bad), np.nonzero(~(ok ^ bad))[0]                              # every restated row is clearly one or the other
        np.testing.assert_array_equal(valid, ok)
        rows = host(plan.icrf)
        print(f"b={b} S={S} P={P} g={g}: taken={int(ref['taken'].sum())} replaced={int(ref['replaced'].sum())} invalid={int(bad.sum())} "
              f"max|trial - ref|={np.abs(trial - ref['trial']).max():.3e} max|row - ref|={np.abs(rows - icrfs).max():.3e}")
        np.testing.assert_allclose(rows, icrfs, rtol=0, atol=1e-13)
        assert np.all(rows[:, 0] == 0.0) and np.all(rows[:, -1] == 1.0)
        np.testing.assert_array_equal(host(plan.valid).astype(bool), valid)
        n_invalid += int((~valid).sum())
        Et = host(plan.trial_energies)
        assert np.all(np.isposinf(Et[~valid]))
        e_ref = host(energies_of(pr, plan.icrf, valid))                                  # the same entry on the same rows: the same bits
        np.testing.assert_array_equal(Et[valid].view(np.int64), e_ref[valid].view(np.int64))
        # selection, statistics and stop flag, given those energies
        pop2, E2, best2, mean, sd, stop, _ = np_select(pop, E, trial, Et, g)
        st = plan.read_status()
        np.testing.assert_array_equal(host(plan.population), pop2)
        np.testing.assert_array_equal(host(plan.energies), E2)
        assert st["best_index"] == best2 and st["best_energy"] == E2[best2] and st["stop"] == stop and st["generation"] == g
        np.testing.assert_allclose(st["mean"], mean, rtol=1e-12)
        np.testing.assert_allclose(st["std"], sd, rtol=1e-12, equal_nan=True)
    assert S < 64 or n_replaced > 0
    assert S < 64 or P == 1 or n_invalid > 0                                             # (one component leaves every row valid)


GENERATION_CASES = [(b, S, P) for b in (9, 12, 16) for S, P in ((8, 1), (64, 3), (128, 5))]


@pytest.mark.parametrize("b,S,P", GENERATION_CASES)
def test_one_generation_matches_restatement(b, S, P):
    check_one_generation("cpu", b, S, P)


# ------------------------------------------------------------------------------------------------ 2: borders of the row walk
def check_row_walk_borders(device, b):
    """pca = 0 and mean[-1] == 1: `last` is 1, the shift 0, the row IS the mean ICRF - a tie in it survives exactly, wherever the left
    neighbour comes from (the wave, another wave, another segment)."""
    pr = make_problem(device, b, P=1)
    n = pr["n"]
    pca = np.zeros((n, 1))
    pop = np.random.default_rng(b).random((8, 1))
    straight = np.linspace(0, 1, n)
    assert straight[-1] == 1.0 and np.all(np.diff(straight) > 0)

    def verdicts(mean):
        plan = make_plan(pr, pop, mean=mean, pca=pca)
        plan.launch()
        np.testing.assert_array_equal(host(plan.icrf), np.tile(mean, (8, 1)))
        return host(plan.valid)
    assert np.all(verdicts(straight) == 1)
    for d in (1, 64, 255, 256, 257, 320, n - 1):
        mean = straight.copy()
        if d == n - 1:
            mean[d - 1] = mean[d]                                                        # (mean[-1] stays 1)
        else:
            mean[d] = mean[d - 1]
        assert mean[-1] == 1.0 and np.count_nonzero(np.diff(mean) <= 0) == 1
        assert np.all(verdicts(mean) == 0), d


@pytest.mark.parametrize("b", [9, 10])
def test_row_walk_borders(b):
    check_row_walk_borders("cpu", b)


# ------------------------------------------------------------------------------------------------ 3: the 8-bit entry's mutation stage
def check_same_trial_as_8_bit(device, b=12):
    pr8, pr = de.make_problem(device, *SHAPE), make_problem(device, b)
    pop = np.random.default_rng(5).random((32, 3))
    for g in (1, 7):
        plans = [de.make_plan(pr8, pop, seed=77), make_plan(pr, pop, seed=77)]
        for plan in plans:
            plan.launch()
            poke(plan, nat.HM_DE_BEST_INDEX, 3)
            poke(plan, nat.HM_DE_GENERATION, g)
            poke(plan, nat.HM_DE_STOP, 0)
            np.testing.assert_array_equal(host(plan.population), pop)
            plan.launch()
        t8, t16 = host(plans[0].trial), host(plans[1].trial)
        assert not np.array_equal(t8, pop) and t8.tobytes() == t16.tobytes(), g


def test_same_trial_as_the_8_bit_entry():
    check_same_trial_as_8_bit("cpu")


# ------------------------------------------------------------------------------------------------ 4: determinism
def solve_state(pr, seed, check_every, graph=True, max_iterations=5, S=32, variant=0):
    rng = np.random.default_rng(3)
    pop = rng.random((S, 3))
    pop[: S // 2] = near_optimum(pr, rng, S // 2, 0.2)
    plan = make_plan(pr, pop, seed=seed, max_generations=2 * max_iterations, variant=variant)
    st = plan.run(check_every, graph)
    return host(plan.population), host(plan.energies), host(plan.trial), st


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def check_determinism(device, b=12):
    pr = make_problem(device, b)
    first = solve_state(pr, 7, 8)
    assert same(solve_state(pr, 7, 8), first)
    assert first[3]["generation"] == 10 and first[3]["stop"] & nat.HM_DE_STOP_MAX       # 11 launches of 16 ran, 5 were no-ops
    for ce in (1, 2, 3):
        assert same(solve_state(pr, 7, ce), first), ce
    assert not np.array_equal(solve_state(pr, 8, 8)[2], first[2])                        # another seed: other trials
    for variant in (1, 2):
        assert same(solve_state(pr, 7, 8, variant=variant), first), variant
    # variant 1 where the row does not fit LDS: the energy entry's status, before any launch
    pr16 = make_problem(device, 16)
    plan = make_plan(pr16, np.full((8, 3), 0.5), variant=1)
    with pytest.raises(NotImplementedError, match="hm_de_generation_u16"):
        plan.launch()
    assert plan.read_status()["evaluations"] == 0
    return first


def test_determinism_check_every_and_variants():
    check_determinism("cpu")


# ------------------------------------------------------------------------------------------------ 5: stopping
def check_stopping(device, b=10):
    pr = make_problem(device, b)
    rng = np.random.default_rng(4)
    near = near_optimum(pr, rng, 16, 0.04)                                               # every member valid: finite energies throughout
    plan = make_plan(pr, near, tol=1e9)
    st = plan.run(8)
    assert np.all(np.isfinite(host(plan.energies)))
    assert st["generation"] == 2 and st["stop"] == nat.HM_DE_STOP_CONVERGED              # a huge tol: the first pass (two generations)
    plan = make_plan(pr, near, tol=0.0, max_generations=6)
    st = plan.run(8)
    assert st["generation"] == 6 and st["stop"] == nat.HM_DE_STOP_MAX
    # frozen: after the stop flag further launches move nothing
    state = lambda: [host(x).tobytes() for x in (plan.population, plan.energies, plan.trial, plan.icrf, plan.valid, plan.status)]  # noqa: E731
    before = state()
    for _ in range(3):
        plan.launch()
    assert state() == before
    plan = make_plan(pr, near, tol=0.0, energy_limit=1e9)
    st = plan.run(8)
    assert st["generation"] == 2 and st["stop"] == nat.HM_DE_STOP_ENERGY
    # energies that include +inf never count as converged, whatever tol
    corner = 0.02 * rng.random((16, 3))                                                  # x near (-1, -1, -1): no valid row
    plan = make_plan(pr, corner, tol=1e9, max_generations=4)
    st = plan.run(8)
    assert np.isinf(host(plan.energies)).any()
    assert st["generation"] == 4 and st["stop"] == nat.HM_DE_STOP_MAX and not np.isfinite(st["mean"])
    # the same through solve_channel_u16
    args = (pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0, b)
    assert ic.solve_channel_u16(*args, seed=7, max_iterations=3)[2] == 3
    assert ic.solve_channel_u16(*args, seed=7, max_iterations=30, energy_limit=1e9)[2] == 1


def test_stopping_and_frozen_state():
    check_stopping("cpu")


# ------------------------------------------------------------------------------------------------ 7: end to end
def check_end_to_end(device, b=10):
    pr = make_problem(device, b, channels=3)
    n, limits = pr["n"], (pr["lower"], pr["upper"])
    assert len(pr["stacks"]) == 3
    args = (pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0)
    e0 = ic._energy_function(np.zeros(3), pr["mean"], pr["pca"], pr["stack"], None, limits[0], limits[1], True, pr["t"], b)
    # the bound is one SciPy's solver - the reference path - meets on this input, from the same seed
    _, e_scipy, _ = ic.solve_channel(*args, data_limits=limits, seed=7, max_iterations=40, vectorized=True, bit_depth=b)
    print(f"SciPy seed 7: e0={e0:.6e} e={e_scipy:.6e}")
    assert e_scipy < e0 / 10, (e_scipy, e0)
    icrf, e, n_it = ic.solve_channel_u16(*args, b, data_limits=limits, seed=7, max_iterations=40)
    print(f"solve_channel_u16 seed 7: e={e:.6e} after {n_it} iterations")
    assert icrf.shape == (n,) and n_it <= 40
    assert e < e0 / 10, (e, e0)
    # the returned ICRF is the best member's candidate (before the shift of the energy function)
    shifted = icrf + (1 - icrf[-1])
    shifted[0] = 0
    np.testing.assert_allclose(host(energies_of(pr, shifted[None], None))[0], e, rtol=1e-12)
    assert ic.solve_channel_u16(*args, b, seed=7, max_iterations=2)[2] == 2              # default limits: the 8-bit ones at this depth
    table, energies = ic.calibration_u16([pr["mean"]] * 3, [pr["pca"]] * 3, pr["stacks"], [None] * 3, pr["t"], -1.0, 1.0, b,
                                         data_limits=limits, max_iterations=10)
    assert table.shape == (n, 3) and energies.shape == (3,) and np.all(np.isfinite(energies))
    assert table.min() >= 0 and table.max() <= 1 and np.all(table[0] == 0) and np.all(table[-1] == 1)
    out = eng(device).merge([torch.from_numpy(f).to(device) for f in pr["frames"]], pr["t"], table, bit_depth=b)
    assert out["val"].shape == SHAPE[:2] + (3,) and bool(torch.isfinite(out["val"]).any())
    # restarts: never worse than any of its seeds alone
    singles = [ic.solve_channel_u16(*args, b, data_limits=limits, seed=ic.restart_seed(7, r), max_iterations=6)[1] for r in range(3)]
    e3 = ic.solve_channel_u16(*args, b, data_limits=limits, seed=7, max_iterations=6, restarts=3)[1]
    assert e3 == min(singles) and all(e3 <= s for s in singles)


def test_end_to_end():
    check_end_to_end("cpu")


# ------------------------------------------------------------------------------------------------ 8: argument rules and API
EINVAL, ESHAPE, EUNSUP, EALIGN = nat.HM_EINVAL, nat.HM_ESHAPE, nat.HM_EUNSUPPORTED, nat.HM_EALIGN


@pytest.mark.parametrize("which", ["hip", "host"])
def test_abi_rejects_bad_arguments_without_a_device(which):
    """Every status of hm_de_generation_u16 in the header's order, alone, from the argument checks: every refusal returns before any
    launch, so the device library answers on fake host pointers (a launch attempt without a GPU would be HM_ELAUNCH)."""
    lib = nat.hip_lib if which == "hip" else nat.host_lib()
    fake = 0x7f0000000000
    t = (C.c_double * 5)(1, 2, 4, 8, 16)

    def call(S=16, P=3, N=5, null=(), dn=None, **kw):
        ptrs = [None if i in null else fake + 4096 * i for i in range(13)]
        if dn is not None:
            ptrs[11] = dn
        sc = dict(n_pixels=100, lower=80, upper=4000, seed=7, max_gen=10, m_lo=0.0, m_hi=1.95, cr=0.4, tol=0.01, e_lim=0.0, bits=12, variant=0)
        sc.update(kw)
        return lib.hm_de_generation_u16(*ptrs, t, sc["n_pixels"], N, sc["lower"], sc["upper"], S, P, sc["seed"], sc["max_gen"], sc["m_lo"],
                                        sc["m_hi"], sc["cr"], sc["tol"], sc["e_lim"], sc["bits"], sc["variant"], fake + (1 << 20), None)
    # hm_de_generation's, in its order
    assert call(S=3) == EINVAL and call(S=-1) == EINVAL and call(P=0) == EINVAL
    assert call(max_gen=-1) == EINVAL and call(n_pixels=-1) == EINVAL
    assert call(S=nat.HM_DE_MAX_POP + 1) == ESHAPE and call(P=nat.HM_DE_MAX_PARAMS + 1) == ESHAPE
    assert call(N=1) == ESHAPE and call(N=nat.HM_MAX_FRAMES + 1) == ESHAPE
    assert call(m_hi=2.0) == EINVAL and call(m_lo=1.0, m_hi=0.5) == EINVAL
    assert call(cr=float("nan")) == EINVAL and call(cr=1.5) == EINVAL
    assert call(tol=-1.0) == EINVAL and call(tol=float("nan")) == EINVAL and call(e_lim=float("nan")) == EINVAL
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11):                                     # every state / model buffer and the stack (std is nullable)
        assert call(null=(i,)) == EINVAL, i
    # the energy stage's, for depth, variant and limits
    assert call(bits=8) == EINVAL and call(bits=17) == EINVAL
    assert call(variant=3) == EINVAL and call(variant=-1) == EINVAL
    assert call(lower=-1) == EINVAL and call(upper=4096) == EINVAL and call(bits=9, upper=512) == EINVAL
    assert call(bits=15, variant=1) == EUNSUP and call(bits=16, variant=1) == EUNSUP
    assert call(dn=fake + 4096 * 11 + 1) == EALIGN
    # an earlier rule wins
    assert call(S=nat.HM_DE_MAX_POP + 1, bits=8) == ESHAPE and call(bits=15, variant=1, upper=1 << 15) == EINVAL
    assert call(bits=15, variant=1, dn=fake + 1) == EUNSUP and call(null=(0,), bits=8) == EINVAL
    if which == "hip":
        assert lib.hm_de_generation_u16(*[fake + 4096 * i for i in range(13)], t, 100, 5, 80, 4000, 16, 3, 7, 10, 0.0, 1.95, 0.4, 0.01, 0.0,
                                        12, 0, None, None) == EINVAL                     # the device build's own: a NULL workspace, last
        if not torch.cuda.is_available():
            assert call() == nat.HM_ELAUNCH and call(bits=16, upper=65535) == nat.HM_ELAUNCH   # valid arguments meet no device
    # the 8-bit entry's limit rule is what it was
    ptrs = [fake + 4096 * i for i in range(13)]
    assert lib.hm_de_generation(*ptrs, t, 100, 5, 5, 256, 16, 3, 7, 10, 0.0, 1.95, 0.4, 0.01, 0.0, fake + (1 << 20), None) == EINVAL


def check_plan_refusals(device):
    pr, pr8 = make_problem(device, 12), de.make_problem(device, *SHAPE)
    e, pop = eng(device), np.full((16, 3), 0.5)

    def plan(stack=pr["stack"], mean=pr["mean"], pca=pr["pca"], pop=pop, lower=pr["lower"], upper=pr["upper"], b=12, **kw):
        return e.DEPlanU16(stack, None, pr["t"], mean, pca, -1.0, 1.0, pop, lower, upper, 11, 10, bit_depth=b, **kw)
    p = plan()
    assert p.S == 16 and p.bit_depth == 12 and tuple(p.icrf.shape) == (16, 4096)
    with pytest.raises(TypeError, match="uint16"):
        plan(stack=pr8["stack"])                                                         # uint8 DNs
    with pytest.raises(TypeError, match="uint16"):
        plan(stack=pr["stack"].to(torch.float64))
    with pytest.raises(ValueError, match="bit_depth"):
        plan(b=None)
    for bad in (8, 17, 12.0, True):
        with pytest.raises(ValueError, match="bit_depth"):
            plan(b=bad)
    with pytest.raises(ValueError, match=r"mean ICRF must have 4096 entries and the PCA basis must be \(4096, 3\)"):
        plan(mean=pr8["mean"], pca=pr8["pca"])                                           # rows of another depth
    with pytest.raises(ValueError, match=r"mean ICRF must have 4096 entries and the PCA basis must be \(4096, 3\)"):
        plan(pca=pr["pca"][:, :2])
    with pytest.raises(ValueError, match=r"mean ICRF must have 2048 entries"):
        plan(b=11, upper=2000)
    for lower, upper in ((-1, 4000), (80, 4096)):
        with pytest.raises(ValueError, match="lower and upper"):
            plan(lower=lower, upper=upper)
    with pytest.raises(ValueError, match="variant"):
        plan(variant=3)
    with pytest.raises(ValueError, match=r"population must be \(S, P\)"):
        plan(pop=pop[0])
    with pytest.raises(ValueError, match=r"3D array with shape \(X, Y, N\)"):
        plan(stack=pr["stack"][0])
    with pytest.raises(ValueError):
        p.run(0)
    with pytest.raises(ValueError, match="mean ICRF"):
        ic.calibration_u16([None], [pr["pca"]], pr["stacks"], [None], pr["t"], -1.0, 1.0, 12)
    with pytest.raises(ValueError, match="bit_depth"):
        ic.solve_channel_u16(pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0, 8)
    # the pinned refusals of the 8-bit names still raise
    with pytest.raises(TypeError, match="image_value_stack must be uint8 digital numbers"):
        e.DEPlan(pr["stack"], None, pr["t"], pr["mean"], pr["pca"], -1.0, 1.0, pop, 5, 250, 1, 10)
    for kw in (dict(solver="device"), dict(solver="device", restarts=2)):
        with pytest.raises(NotImplementedError, match='solver="scipy"'):
            ic.solve_channel(pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0, bit_depth=12, **kw)
    for kw in (dict(solver="device"), dict(solver="device", batched=True), dict(solver="device", restarts=2)):
        with pytest.raises(NotImplementedError, match='solver="scipy"'):
            ic.calibration([pr["mean"]], [pr["pca"]], pr["stacks"], [None], pr["t"], -1.0, 1.0, bit_depth=12, **kw)


def test_plan_refusals():
    check_plan_refusals("cpu")
    pr = make_problem("cpu", 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                           # host tensors outside host_mode(): the HIP backend refuses
        engine.DEPlanU16(pr["stack"], None, pr["t"], pr["mean"], pr["pca"], -1.0, 1.0, np.full((8, 3), 0.5), 80, 4000, 1, 10, bit_depth=12)


def test_host_stack_never_reaches_the_hip_library():
    pr = make_problem("cpu", 10)
    hip, h = nat.hip_lib.calls, nat.host_lib().calls
    before = (hip["hm_de_generation_u16"], hip["hm_linearity_energy_u16"], hip["hm_de_generation"], h["hm_de_generation_u16"], h["hm_de_generation"])
    ic.solve_channel_u16(pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0, 10, seed=7, max_iterations=2)
    assert (hip["hm_de_generation_u16"], hip["hm_linearity_energy_u16"], hip["hm_de_generation"]) == before[:3]
    assert h["hm_de_generation_u16"] >= before[3] + 5 and h["hm_de_generation"] == before[4]


def test_scipy_path_does_not_touch_the_new_entry():
    pr = make_problem("cpu", 10)
    h = nat.host_lib().calls
    before = h["hm_de_generation_u16"]
    ic.solve_channel(pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0, data_limits=(pr["lower"], pr["upper"]), seed=7,
                     max_iterations=2, bit_depth=10)
    assert h["hm_de_generation_u16"] == before
