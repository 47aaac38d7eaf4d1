"""The differential-evolution generation step (hm_de_generation, engine.DEPlan, solve_channel(solver="device")) on the HOST build, against
a NumPy restatement of the algorithm written from the specification in include/hdrmerge.h (counter-based random numbers in uint64, picks,
mutant, crossover, redraw, candidate ICRF, selection, statistics, stop flag) - not from the C++. The checks are functions of a device name:
tests/test_gpu_de.py runs the same ones on the MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import icrf_calibration as ic

U64 = np.uint64
F_LO, F_HI, CR, TOL = 0.0, 1.95, 0.4, 0.01


# ------------------------------------------------------------------------------------------------ the restatement
def mix64(z):
    z = np.atleast_1d(np.asarray(z, dtype=U64))                  # arrays wrap silently; NumPy scalars would warn
    z = z + U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def uniform(seed, g, i, k):
    """U(g, i, k) for broadcastable integer arrays i, k."""
    key = mix64(U64(seed & 0xFFFFFFFFFFFFFFFF) ^ mix64(g))
    i = np.asarray(i, dtype=np.int64).astype(U64)
    k = np.asarray(k, dtype=np.int64).astype(U64)
    r = mix64(key + ((i + U64(1)) << U64(20)) + k)
    return (r >> U64(11)).astype(np.float64) * 2.0 ** -53


def np_trial(pop, best, g, seed, f_lo=F_LO, f_hi=F_HI, cr=CR):
    """-> dict(trial, taken (component came from the mutant), replaced (out-of-range redraw), mutant, F, r0, r1)."""
    S, P = pop.shape
    i, j = np.arange(S), np.arange(P)
    F = f_lo + (f_hi - f_lo) * uniform(seed, g, S, 0)[0]
    a = np.floor(uniform(seed, g, i, 0) * (S - 1)).astype(np.int64)
    r0 = a + (a >= i)
    c = np.floor(uniform(seed, g, i, 1) * (S - 2)).astype(np.int64)
    lo2, hi2 = np.minimum(i, r0), np.maximum(i, r0)
    c = c + (c >= lo2)
    c = c + (c >= hi2)
    r1 = c
    assert np.all(r0 != i) and np.all(r1 != i) and np.all(r0 != r1) and r0.max() < S and r1.max() < S and min(r0.min(), r1.min()) >= 0
    v = pop + F * (pop[best] - pop + pop[r0] - pop[r1])
    fill = np.floor(uniform(seed, g, i, 2) * P).astype(np.int64)
    taken = (uniform(seed, g, i[:, None], 3 + j[None, :]) < cr) | (j[None, :] == fill[:, None])
    replaced = taken & ((v < 0) | (v > 1))
    redraw = uniform(seed, g, i[:, None], 3 + P + j[None, :])
    trial = np.where(taken, np.where(replaced, redraw, v), pop)
    return dict(trial=trial, taken=taken, replaced=replaced, mutant=v, F=F, r0=r0, r1=r1, redraw=redraw)


def np_select(pop, E, trial, Et, g, tol=TOL, energy_limit=0.0, max_generations=1 << 40):
    """-> (population, energies, best index, mean, std, stop flag) after the deferred selection of generation g."""
    acc = np.ones(len(E), bool) if g == 0 else Et <= E
    pop2, E2 = np.where(acc[:, None], trial, pop), np.where(acc, Et, E)
    with np.errstate(invalid="ignore"):
        mean, sd = np.mean(E2), np.std(E2)
    stop = 0
    if g > 0 and g % 2 == 0:
        if np.all(np.isfinite(E2)) and sd <= tol * abs(mean):
            stop |= nat.HM_DE_STOP_CONVERGED
        if E2.min() < energy_limit:
            stop |= nat.HM_DE_STOP_ENERGY
    if g >= max_generations:
        stop |= nat.HM_DE_STOP_MAX
    return pop2, E2, int(np.argmin(E2)), mean, sd, stop, acc


# ------------------------------------------------------------------------------------------------ the problem
def make_problem(device, X=24, Y=24, N=5, P=3, channels=1):
    """The synthetic camera of test_calibration_recovers_response / test_host_calibration_recovers_response, with P PCA components."""
    rng = np.random.default_rng(21)
    t = 1e-3 * 2.0 ** np.arange(N)
    xs = np.linspace(0, 1, 256)
    pca = np.stack([np.sin(np.pi * (m + 1) * xs) / (m + 1) for m in range(P)], axis=1) * 0.1
    mean_icrf = xs ** 2.0
    true_params = np.array([0.6, -0.3, 0.2, 0.1, -0.1][:P])
    true_icrf, ok = ic.candidate_icrfs(true_params, mean_icrf, pca)
    assert ok[0]
    rad = rng.random((X, Y)) * 2.5 / t[-1]
    lin = np.clip(rad[..., None] * t, 0, 1)
    dn = np.clip(np.around(np.interp(lin, true_icrf[0], xs) * 255), 0, 255).astype(np.uint8)
    stacks, stds, tt = ic.initialize_channel_image_stacks([dn[:, :, None, i].repeat(channels, 2) for i in range(N)], t, None, 1, device=device)
    return dict(stacks=stacks, stack=stacks[0], t=tt, pca=pca, mean=mean_icrf, true=true_params, P=P, device=device)


def make_plan(pr, pop, seed=11, max_generations=1 << 40, tol=TOL, energy_limit=0.0):
    eng = ic._engine_for(pr["stack"])
    return eng.DEPlan(pr["stack"], None, pr["t"], pr["mean"], pr["pca"], -1.0, 1.0, pop, 5, 250, seed, max_generations, (F_LO, F_HI), CR,
                      tol, energy_limit)


def energies_of(pr, icrfs, valid):
    return ic._engine_for(pr["stack"]).linearity_energy(pr["stack"], None, pr["t"], icrfs, 5, 250, valid, True).cpu().numpy()


def host(t):
    return t.cpu().numpy().copy()


def poke(plan, word, value):
    plan.status[word] = int(value)


# ------------------------------------------------------------------------------------------------ 1: one generation
def check_one_generation(device, S, P, shape):
    pr = make_problem(device, *shape, P=P)
    rng = np.random.default_rng(100 * S + P)
    pop0 = rng.random((S, P))
    pop0[: S // 2] = 0.5 * (pr["true"] + 1) + 0.1 * (rng.random((S // 2, P)) - 0.5)      # half of the members near the optimum: valid rows
    plan = make_plan(pr, pop0, seed=1234 + S)
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
        print(f"S={S} P={P} g={g}: F={ref['F']:.6f} taken={int(ref['taken'].sum())} replaced={int(ref['replaced'].sum())} "
              f"max|trial - ref|={np.abs(trial - ref['trial']).max():.3e}")
        keep = ~ref["taken"]
        np.testing.assert_array_equal(trial[keep], pop[keep])                            # crossover mask and fill point: exact
        assert ref["taken"].any(axis=1).all()
        np.testing.assert_array_equal(trial[ref["replaced"]], ref["redraw"][ref["replaced"]])   # out-of-range replacements: exact draws
        np.testing.assert_allclose(trial, ref["trial"], rtol=0, atol=1e-14)
        n_replaced += int(ref["replaced"].sum())
        # candidate ICRFs and verdicts of the DEVICE's trial rows
        icrfs, valid = ic.candidate_icrfs(-1.0 + trial * 2.0, pr["mean"], pr["pca"])
        assert np.all(icrfs[:, 255] == 1.0) and np.all(icrfs[:, 0] == 0.0)
        inner = icrfs[:, 1:255]
        assert np.abs(inner).min() > 1e-9 and np.abs(inner - 1).min() > 1e-9             # no entry within 1e-9 of the range limits
        assert np.abs(np.diff(icrfs, axis=1)).min() > 1e-9                               # no step within 1e-9 of zero
        np.testing.assert_allclose(host(plan.icrf), icrfs, rtol=0, atol=1e-13)
        np.testing.assert_array_equal(host(plan.valid).astype(bool), valid)
        n_invalid += int((~valid).sum())
        Et = host(plan.trial_energies)
        assert np.all(np.isinf(Et[~valid]))
        e_ref = energies_of(pr, host(plan.icrf), valid)
        np.testing.assert_allclose(Et[valid], e_ref[valid], rtol=1e-12)
        # selection, statistics and stop flag, given those energies
        pop2, E2, best2, mean, sd, stop, _ = np_select(pop, E, trial, Et, g)
        st = plan.read_status()
        np.testing.assert_array_equal(host(plan.population), pop2)
        np.testing.assert_array_equal(host(plan.energies), E2)
        assert st["best_index"] == best2 and st["best_energy"] == E2[best2] and st["stop"] == stop and st["generation"] == g
        np.testing.assert_allclose(st["mean"], mean, rtol=1e-12)
        np.testing.assert_allclose(st["std"], sd, rtol=1e-12, equal_nan=True)
    assert S < 64 or (n_replaced > 0 and n_invalid > 0)                                  # both branches were exercised


@pytest.mark.parametrize("S,P", [(8, 1), (8, 3), (64, 3), (64, 5), (128, 1), (128, 5)])
def test_one_generation_matches_restatement(S, P):
    check_one_generation("cpu", S, P, (24, 24, 5))


def test_best_index_ties_go_to_the_lowest_index():
    check_ties("cpu", (24, 24, 5))


def check_ties(device, shape):
    """Equal members have equal energies: the best index is the first of them."""
    pr = make_problem(device, *shape)
    pop = np.tile(0.5 * (pr["true"] + 1), (8, 1))
    pop[0] += 0.2
    plan = make_plan(pr, pop)
    plan.launch()
    E = host(plan.energies)
    assert np.all(E[1:] == E[1]) and E[1] < E[0]
    assert plan.read_status()["best_index"] == 1


# ------------------------------------------------------------------------------------------------ 2: many generations
def check_many_generations(device, shape, S=64, seed=5, generations=20):
    pr = make_problem(device, *shape)
    rng = np.random.default_rng(9)
    pop = rng.random((S, 3))
    pop[: S // 2] = 0.5 * (pr["true"] + 1) + 0.2 * (rng.random((S // 2, 3)) - 0.5)
    plan = make_plan(pr, pop, seed=seed, tol=0.0)
    # the restatement, with the existing energy entry point as its energy function
    icrfs, valid = ic.candidate_icrfs(-1.0 + pop * 2.0, pr["mean"], pr["pca"])
    E = energies_of(pr, icrfs, valid)
    plan.launch()
    np.testing.assert_allclose(host(plan.energies), E, rtol=1e-12)
    accepted = 0
    for g in range(1, generations + 1):
        ref = np_trial(pop, int(np.argmin(E)), g, seed)
        icrfs, valid = ic.candidate_icrfs(-1.0 + ref["trial"] * 2.0, pr["mean"], pr["pca"])
        Et = energies_of(pr, icrfs, valid)
        pop, E_new, _, _, _, _, acc = np_select(pop, E, ref["trial"], Et, g, tol=0.0)
        before = host(plan.energies)
        plan.launch()
        acc_dev = host(plan.trial_energies) <= before
        assert np.array_equal(acc_dev, acc), (g, np.nonzero(acc_dev != acc)[0])
        accepted += int(acc.sum())
        E = E_new
    print(f"{generations} generations, S={S}: {accepted} accepted trials, best {E.min():.6e}, "
          f"max rel energy difference {np.nanmax(np.abs(host(plan.energies) - E) / E):.3e}")
    assert 0 < accepted < generations * S
    fin = np.isfinite(E)
    np.testing.assert_array_equal(np.isfinite(host(plan.energies)), fin)
    np.testing.assert_allclose(host(plan.energies)[fin], E[fin], rtol=1e-10)
    np.testing.assert_allclose(host(plan.population), pop, rtol=0, atol=1e-10)
    assert plan.read_status()["generation"] == generations and plan.read_status()["evaluations"] == (generations + 1) * S


def test_twenty_generations_follow_the_restatement():
    check_many_generations("cpu", (24, 24, 5))


# ------------------------------------------------------------------------------------------------ 3: determinism
def solve_state(pr, seed, check_every, graph=True, max_iterations=5, S=32):
    rng = np.random.default_rng(3)
    pop = rng.random((S, 3))
    pop[: S // 2] = 0.5 * (pr["true"] + 1) + 0.2 * (rng.random((S // 2, 3)) - 0.5)
    plan = make_plan(pr, pop, seed=seed, max_generations=2 * max_iterations)
    st = plan.run(check_every, graph)
    return host(plan.population), host(plan.energies), host(plan.trial), st


def check_determinism(device, shape):
    pr = make_problem(device, *shape)
    p1, e1, t1, s1 = solve_state(pr, 7, 8)
    p2, e2, t2, s2 = solve_state(pr, 7, 8)
    assert p1.tobytes() == p2.tobytes() and e1.tobytes() == e2.tobytes() and s1 == s2
    assert s1["generation"] == 10 and s1["stop"] & nat.HM_DE_STOP_MAX                  # 11 launches of 16 ran, 5 were no-ops
    for ce in (1, 2, 3):
        p3, e3, t3, s3 = solve_state(pr, 7, ce)
        assert p3.tobytes() == p1.tobytes() and e3.tobytes() == e1.tobytes() and t3.tobytes() == t1.tobytes() and s3 == s1, ce
    p4, e4, t4, s4 = solve_state(pr, 8, 8)
    assert not np.array_equal(t4, t1)                                                    # another seed: other trials
    return p1, e1, t1, s1


def test_determinism_and_check_every():
    check_determinism("cpu", (24, 24, 5))


# ------------------------------------------------------------------------------------------------ 4: stopping
def check_stopping(device, shape):
    pr = make_problem(device, *shape)
    rng = np.random.default_rng(4)
    near = 0.5 * (pr["true"] + 1) + 0.04 * (rng.random((16, 3)) - 0.5)                  # every member valid: finite energies throughout
    plan = make_plan(pr, near, tol=1e9)
    st = plan.run(8)
    assert np.all(np.isfinite(host(plan.energies)))
    assert st["generation"] == 2 and st["stop"] == nat.HM_DE_STOP_CONVERGED              # a huge tol: the first pass (two generations)
    plan = make_plan(pr, near, tol=0.0, max_generations=6)
    st = plan.run(8)
    assert st["generation"] == 6 and st["stop"] == nat.HM_DE_STOP_MAX
    plan = make_plan(pr, near, tol=0.0, energy_limit=1e9)
    st = plan.run(8)
    assert st["generation"] == 2 and st["stop"] == nat.HM_DE_STOP_ENERGY
    # energies that include +inf never count as converged, whatever tol
    corner = 0.02 * rng.random((16, 3))                                                  # x near (-1, -1, -1): no valid row
    plan = make_plan(pr, corner, tol=1e9, max_generations=4)
    st = plan.run(8)
    assert np.isinf(host(plan.energies)).any()
    assert st["generation"] == 4 and st["stop"] == nat.HM_DE_STOP_MAX and not np.isfinite(st["mean"])
    # the same through solve_channel
    args = (pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0)
    assert ic.solve_channel(*args, seed=7, max_iterations=3, solver="device")[2] == 3
    assert ic.solve_channel(*args, seed=7, max_iterations=30, energy_limit=1e9, solver="device")[2] == 1


def test_stopping():
    check_stopping("cpu", (24, 24, 5))


# ------------------------------------------------------------------------------------------------ 5: end to end
def check_end_to_end(device, shape):
    pr = make_problem(device, *shape, channels=3)
    assert len(pr["stacks"]) == 3
    args = (pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0)
    e0 = ic._energy_function(np.zeros(3), pr["mean"], pr["pca"], pr["stack"], None, 5, 250, True, pr["t"])
    icrf, e, n_it = ic.solve_channel(*args, seed=7, max_iterations=40, solver="device")
    print(f"solver='device' seed 7: e0={e0:.6e} e={e:.6e} after {n_it} iterations")
    assert icrf.shape == (256,) and n_it <= 40
    assert e < e0 / 10, (e, e0)
    # the returned ICRF is the best member's candidate (before the shift of the energy function)
    shifted = icrf + (1 - icrf[-1])
    shifted[0] = 0
    np.testing.assert_allclose(energies_of(pr, shifted[None], None)[0], e, rtol=1e-12)
    table, energies = ic.calibration([pr["mean"]] * 3, [pr["pca"]] * 3, pr["stacks"], [None] * 3, pr["t"], -1.0, 1.0, max_iterations=10,
                                     solver="device")
    assert table.shape == (256, 3) and energies.shape == (3,) and np.all(np.isfinite(energies))
    assert table.min() >= 0 and table.max() <= 1 and np.all(table[0] == 0) and np.all(table[-1] == 1)


def test_end_to_end():
    check_end_to_end("cpu", (24, 24, 5))


# ------------------------------------------------------------------------------------------------ 6: errors and API
def test_default_solver_is_scipy_and_unchanged():
    import inspect
    assert inspect.signature(ic.solve_channel).parameters["solver"].default == "scipy"
    assert inspect.signature(ic.calibration).parameters["solver"].default == "scipy"
    assert inspect.signature(ic.solve_channel).parameters["check_every"].default == 8
    pr = make_problem("cpu")
    args = (pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0)
    h = nat.host_lib()
    de_calls = h.calls["hm_de_generation"]
    a = ic.solve_channel(*args, seed=7, max_iterations=4)
    b = ic.solve_channel(*args, seed=7, max_iterations=4, solver="scipy")
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    assert h.calls["hm_de_generation"] == de_calls                                      # the SciPy path does not touch the new entry point


def test_solver_argument_errors():
    pr = make_problem("cpu")
    args = (pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0)
    with pytest.raises(ValueError, match="solver"):
        ic.solve_channel(*args, solver="cupy")
    with pytest.raises(NotImplementedError, match='solver="scipy"'):
        ic.solve_channel(np.linspace(0, 1, 256), pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0, use_mean_ICRF=False, solver="device")
    with pytest.raises(NotImplementedError, match='solver="scipy"'):
        ic.calibration([None], [pr["pca"]], pr["stacks"], [None], pr["t"], -1.0, 1.0, initial_function=np.linspace(0, 1, 256), solver="device")
    with pytest.raises(ValueError):
        make_plan(pr, np.full((16, 3), 0.5)).run(0)
    # the stack / std stack / exposure checks that DEPlan and linearity_energy share, and DEPlan's own model checks
    eng, pop, icrfs = ic._engine_for(pr["stack"]), np.full((16, 3), 0.5), np.linspace(0, 1, 256)[None]

    def plan(stack=pr["stack"], std=None, t=pr["t"], mean=pr["mean"], pca=pr["pca"], pop=pop):
        return eng.DEPlan(stack, std, t, mean, pca, -1.0, 1.0, pop, 5, 250, 11, 10)

    def energy(stack=pr["stack"], std=None, t=pr["t"]):
        return eng.linearity_energy(stack, std, t, icrfs, 5, 250)
    assert plan().S == 16 and energy().shape == (1,)
    sd = torch.full(tuple(pr["stack"].shape), 0.01, dtype=torch.float64)
    assert plan(std=sd).std is not None and energy(std=sd).shape == (1,)
    for build in (plan, energy):
        with pytest.raises(TypeError, match="must be uint8 digital numbers"):
            build(stack=pr["stack"].to(torch.float64))
        with pytest.raises(ValueError, match=r"3D array with shape \(X, Y, N\)"):
            build(stack=pr["stack"][0])
        with pytest.raises(ValueError, match="exposure_values must be a 1D array matching the third dimension"):
            build(t=pr["t"][:4])
        with pytest.raises(ValueError, match="image_std_stack must be float64 and shaped like image_value_stack"):
            build(std=sd.to(torch.float32))
        with pytest.raises(ValueError, match="image_std_stack must be float64 and shaped like image_value_stack"):
            build(std=sd[:, :-1])
        with pytest.raises(TypeError, match="image_value_stack must be a torch.Tensor"):
            build(stack=pr["stack"].numpy())
    with pytest.raises(ValueError, match=r"population must be \(S, P\)"):
        plan(pop=pop[0])
    with pytest.raises(ValueError, match=r"mean ICRF must have 256 entries and the PCA basis must be \(256, 3\)"):
        plan(mean=pr["mean"][:255])
    with pytest.raises(ValueError, match=r"mean ICRF must have 256 entries and the PCA basis must be \(256, 3\)"):
        plan(pca=pr["pca"][:, :2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):                           # host tensors outside host_mode(): the HIP backend refuses
        ic.engine.DEPlan(pr["stack"], None, pr["t"], pr["mean"], pr["pca"], -1.0, 1.0, pop, 5, 250, 11, 10)


def test_host_stack_never_reaches_the_hip_library():
    pr = make_problem("cpu")
    hip, h = nat.hip_lib.calls, nat.host_lib().calls
    before = (hip["hm_de_generation"], hip["hm_linearity_energy"], h["hm_de_generation"])
    ic.solve_channel(pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0, seed=7, max_iterations=2, solver="device")
    assert (hip["hm_de_generation"], hip["hm_linearity_energy"]) == before[:2]
    assert h["hm_de_generation"] >= before[2] + 5


@pytest.mark.parametrize("which", ["hip", "host"])
def test_abi_rejects_bad_arguments_without_a_device(which):
    """S < 4, S or P over the limits, null state buffers, NaN parameters: HM_EINVAL / HM_ESHAPE from the argument checks alone - on the
    HIP library loaded on a machine without a GPU any launch attempt would be HM_ELAUNCH instead."""
    lib = nat.hip_lib if which == "hip" else nat.host_lib()
    fake = 0x7f0000000000
    t = (C.c_double * 5)(1, 2, 4, 8, 16)

    def call(S=16, P=3, N=5, null=(), **kw):
        ptrs = [None if i in null else fake + 4096 * i for i in range(13)]
        sc = dict(n_pixels=100, lower=5, upper=250, seed=7, max_gen=10, m_lo=0.0, m_hi=1.95, cr=0.4, tol=0.01, e_lim=0.0)
        sc.update(kw)
        return lib.hm_de_generation(*ptrs, t, sc["n_pixels"], N, sc["lower"], sc["upper"], S, P, sc["seed"], sc["max_gen"], sc["m_lo"],
                                    sc["m_hi"], sc["cr"], sc["tol"], sc["e_lim"], fake + (1 << 20), None)
    assert call(S=3) == nat.HM_EINVAL
    assert call(S=-1) == nat.HM_EINVAL
    assert call(S=nat.HM_DE_MAX_POP + 1) == nat.HM_ESHAPE
    assert call(P=nat.HM_DE_MAX_PARAMS + 1) == nat.HM_ESHAPE
    assert call(P=0) == nat.HM_EINVAL
    assert call(N=1) == nat.HM_ESHAPE and call(N=nat.HM_MAX_FRAMES + 1) == nat.HM_ESHAPE
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11):                                     # every state / model buffer and the stack (std is nullable)
        assert call(null=(i,)) == nat.HM_EINVAL, i
    assert call(lower=-1) == nat.HM_EINVAL and call(upper=256) == nat.HM_EINVAL
    assert call(cr=float("nan")) == nat.HM_EINVAL and call(cr=1.5) == nat.HM_EINVAL
    assert call(m_hi=2.0) == nat.HM_EINVAL and call(m_lo=1.0, m_hi=0.5) == nat.HM_EINVAL
    assert call(tol=-1.0) == nat.HM_EINVAL and call(tol=float("nan")) == nat.HM_EINVAL and call(e_lim=float("nan")) == nat.HM_EINVAL
    assert call(max_gen=-1) == nat.HM_EINVAL and call(n_pixels=-1) == nat.HM_EINVAL
    assert lib.hm_de_workspace_bytes(100, 5, 3) == 0
    if which == "hip":
        assert lib.hm_de_workspace_bytes(784, 7, 128) == lib.hm_linearity_energy_workspace_bytes(784, 7, 128) > 0
        if not torch.cuda.is_available():
            assert call() == nat.HM_ELAUNCH                                               # valid arguments meet no device
    assert nat.HM_ABI_VERSION == 2 and lib.hm_version() == 2


def test_rng_restatement_known_values():
    """mix64 is splitmix64's output function: from state 0 the generator's first outputs are the published test vector."""
    assert int(mix64(0)[0]) == 0xE220A8397B1DCDAF
    assert int(mix64(0x9E3779B97F4A7C15)[0]) == 0x6E789E6AA1B965F4
    u = uniform(7, 3, np.arange(1000)[:, None], np.arange(10)[None, :])
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.02
