"""K differential-evolution problems per call for 9- to 16-bit cameras (hm_de_generation_u16_batch, engine.DEBatchPlanU16,
solve_channel_u16(batched=True), calibration_u16(batched=True)) on the HOST build. The specification in include/hdrmerge.h is an equality:
problem k of a batch evolves bit for bit as hm_de_generation_u16 evolves it alone, so every check here compares a batch with K independent
DEPlanU16s built from the same inputs on the same build - bytes of every state array and of the status words, no tolerance. The checks are
functions of a device name: tests/test_gpu_de_u16_batch.py runs the same ones on the MI355X, where the equality is the hard part (the
problem as a grid dimension of the row walk, launch geometry and row placement per problem, the skip of stopped problems).

The cameras are test_de_u16_host.make_problem's (mean ICRF 0.5 xs + 0.5 xs**p) bent a little more for every problem."""
import ctypes as C

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from camera_linearity_amd import icrf_calibration as ic

import test_de_u16_host as du
from test_de_batch_host import STATE, TRUE, assert_batch_equals_singles, populations, same_status
from test_de_host import CR, F_HI, F_LO, host


# ------------------------------------------------------------------------------------------------ problems
def camera(k, P, b):
    """Mean ICRF and PCA basis (2**b rows) of problem k."""
    xs = np.linspace(0, 1, 2 ** b)
    pca = np.stack([np.sin(np.pi * (m + 1) * xs) / (m + 1) for m in range(P)], axis=1) * (0.1 + 0.01 * k)
    return 0.5 * xs + 0.5 * xs ** (2.0 + 0.1 * k), pca


_STACKS = {}


def synthetic_stack(device, shape, seed, mean, pca, b):
    """A (X, Y, N) torch.uint16 stack of the camera (mean, pca, TRUE) at depth b under its own radiance field: computed once per key and
    never changed."""
    key = (str(device), shape, seed, b, mean.tobytes()[:64], pca.shape[1], float(pca[1, 0]))
    if key not in _STACKS:
        X, Y, N = shape
        n = 2 ** b
        rng = np.random.default_rng(seed)
        t = 1e-3 * 2.0 ** np.arange(N)
        xs = np.linspace(0, 1, n)
        true_icrf, ok = ic.candidate_icrfs(TRUE[:pca.shape[1]], mean, pca)
        assert ok[0]
        lin = np.clip((rng.random((X, Y)) * 2.5 / t[-1])[..., None] * t, 0, 1)
        dn = np.clip(np.around(np.interp(lin, true_icrf[0], xs) * (n - 1)), 0, n - 1).astype(np.uint16)
        _STACKS[key] = (torch.from_numpy(dn.view(np.int16)).to(device).view(torch.uint16), t)
    return _STACKS[key]


def random_stack(device, shape, seed, b):
    """Sorted random DNs of depth b and a std stack (the stack of test_de_batch_host.random_stack at depth b)."""
    X, Y, N = shape
    rng = np.random.default_rng(seed)
    dn = np.sort(rng.integers(0, 2 ** b, (X, Y, N)).astype(np.uint16), axis=2)
    sd = torch.as_tensor(0.004 * (1 + rng.random((X, Y, N))), device=device)
    return torch.from_numpy(dn.view(np.int16)).to(device).view(torch.uint16), sd, 1e-3 * 2.0 ** np.arange(N)


def limits(b):
    return 5 << (b - 8), 250 << (b - 8)


def make_batch(device, b, K, shape, S, P, seeds, n_stacks=None, stack_of=None, pop=None, variant=0, **kw):
    """-> dict(stacks, stds, t, means, pcas, pop, seeds, stack_of, b, variant, kw): the inputs of one DEBatchPlanU16 and of its K DEPlanU16s."""
    n_stacks = K if n_stacks is None else n_stacks
    cams = [camera(k, P, b) for k in range(K)]
    stack_of = list(range(K)) if stack_of is None else list(stack_of)
    stacks, t = [], None
    for s in range(n_stacks):
        owner = stack_of.index(s)                                                        # the first problem that reads stack s made it
        dn, t = synthetic_stack(device, shape, 100 + s, *cams[owner], b)
        stacks.append(dn)
    assert len({host(st.view(torch.int16)).tobytes() for st in stacks}) == n_stacks      # distinct data
    return dict(stacks=stacks, stds=None, t=t, means=[c[0] for c in cams], pcas=[c[1] for c in cams],
                pop=populations(K, S, P, 7 * S + P) if pop is None else pop, seeds=list(seeds), stack_of=stack_of, b=b, variant=variant, kw=kw)


def plan_kw(q):
    kw = dict(max_generations=1 << 40, tol=0.0, energy_limit=0.0)
    kw.update(q["kw"])
    return kw


def eng_of(q):
    return ic._engine_for(q["stacks"][0])


def batch_plan(q, explicit_stack_of=True, variant=None):
    kw = plan_kw(q)
    lo, hi = limits(q["b"])
    return eng_of(q).DEBatchPlanU16(q["stacks"], q["stds"], q["t"], q["means"], q["pcas"], -1.0, 1.0, q["pop"], lo, hi, q["seeds"],
                                    kw["max_generations"], (F_LO, F_HI), CR, kw["tol"], kw["energy_limit"],
                                    stack_of=q["stack_of"] if explicit_stack_of else None, bit_depth=q["b"],
                                    variant=q["variant"] if variant is None else variant)


def single_plans(q):
    kw = plan_kw(q)
    lo, hi = limits(q["b"])
    out = []
    for k, c in enumerate(q["stack_of"]):
        sd = None if q["stds"] is None else q["stds"][c]
        out.append(eng_of(q).DEPlanU16(q["stacks"][c], sd, q["t"], q["means"][k], q["pcas"][k], -1.0, 1.0, q["pop"][k], lo, hi, q["seeds"][k],
                                       kw["max_generations"], (F_LO, F_HI), CR, kw["tol"], kw["energy_limit"], q["b"], q["variant"]))
    return out


def step_both(q, generations, explicit_stack_of=True):
    """`generations` + 1 launches (generation 0 evaluates the population) of the batch and of every single plan."""
    batch, singles = batch_plan(q, explicit_stack_of), single_plans(q)
    assert tuple(batch.icrf.shape) == (batch.K, batch.S, 2 ** q["b"])
    for _ in range(generations + 1):
        batch.launch()
        for p in singles:
            p.launch()
    sts = assert_batch_equals_singles(batch, singles)
    assert all(st["generation"] == generations for st in sts)
    return batch, singles


def state_bytes(plan, k=None):
    pick = (lambda x: x) if k is None else (lambda x: x[k])
    return [host(pick(getattr(plan, name))).tobytes() for name in STATE + ("status",)]


# ------------------------------------------------------------------------------------------------ 1: batch equals singles
# depth 9: U = 2, 10: U = 4, 12: U = 8 and one workgroup per member, 14: 8 slabs, 16: 16 slabs of two trips (only (8, 3): 12.6 MB of rows)
EQUAL_CASES = [(b, S, P) for b in (9, 10, 12, 14, 16) for S, P in ((8, 3), (16, 5)) if b < 16 or S == 8]


def check_batch_equals_singles(device, b, S, P):
    q = make_batch(device, b, 3, (40, 40, 6), S, P, seeds=(7, 8, 9))                     # 1600 pixels: two pixel chunks
    batch, singles = step_both(q, 12)
    E = host(batch.energies)
    assert np.isfinite(E).any(axis=1).all() and len({E[k].tobytes() for k in range(3)}) == 3      # three different problems
    assert not np.array_equal(host(batch.trial[0]), host(batch.trial[1]))


@pytest.mark.parametrize("b,S,P", EQUAL_CASES)
def test_batch_equals_singles(b, S, P):
    check_batch_equals_singles("cpu", b, S, P)


# ------------------------------------------------------------------------------------------------ 2: geometry per problem
def check_geometry_is_per_problem(device, b=12):
    """18 496 pixels (> 16 384) and S = 5 (< 8): a single solve takes the pair-major energy kernel. K S = 10 >= 8 would choose the
    pixel-major one, whose sums differ in the last bits."""
    q = make_batch(device, b, 2, (136, 136, 3), 5, 3, seeds=(3, 4), pop=populations(2, 5, 3, 1, spread=0.1))
    batch, _ = step_both(q, 12)
    assert np.isfinite(host(batch.trial_energies)).any()


def test_geometry_rule_is_per_problem():
    check_geometry_is_per_problem("cpu")


# ------------------------------------------------------------------------------------------------ 3: pair-major and std
def check_pair_major_and_std(device, b):
    K, S, P = 2, 16, 3
    q = make_batch(device, b, K, (8, 8, 5), S, P, seeds=(3, 5))                          # (cameras and populations; the stacks follow)
    data = [random_stack(device, (16, 16, 10), 2 + k, b) for k in range(K)]
    rng = np.random.default_rng(2)
    q.update(stacks=[d[0] for d in data], stds=[d[1] for d in data], t=data[0][2],
             pop=0.5 * (TRUE[:P] + 1) + 0.1 * (rng.random((K, S, P)) - 0.5))
    q["kw"] = dict(max_generations=100, tol=0.01)
    batch, _ = step_both(q, 3)
    lo, hi = limits(b)
    for k in range(K):
        valid = host(batch.valid[k]).astype(bool)
        assert valid.any()
        ref = eng_of(q).linearity_energy(q["stacks"][k], q["stds"][k], q["t"], batch.icrf[k], lo, hi, valid, True, bit_depth=b).cpu().numpy()
        np.testing.assert_array_equal(host(batch.trial_energies[k]), ref)


@pytest.mark.parametrize("b", [12, 16])
def test_pair_major_and_std(b):
    check_pair_major_and_std("cpu", b)


# ------------------------------------------------------------------------------------------------ 4: shared stacks
def check_shared_stacks(device, b=12):
    q = make_batch(device, b, 4, (40, 40, 6), 8, 3, seeds=(11, 12, 13, 14), n_stacks=2, stack_of=[0, 0, 1, 1])
    batch, _ = step_both(q, 6)
    assert len({host(batch.energies[k]).tobytes() for k in range(4)}) == 4               # same stack, other seed and camera: another problem


def test_shared_stacks():
    check_shared_stacks("cpu")


# ------------------------------------------------------------------------------------------------ 5: stopping at different times
def check_problems_stop_at_different_times(device, b):
    """At 14 bits the slab walk and the verdict kernel must skip the stopped problem too: its icrf rows and verdicts stay as they were."""
    S, P = 16, 3
    pop = populations(3, S, P, 5)
    pop[0] = 0.5 * (TRUE[:P] + 1)                          # S equal members: the mutant is the member, std(E) = 0 -> converged at generation 2
    q = make_batch(device, b, 3, (40, 40, 6), S, P, seeds=(7, 8, 9), pop=pop, max_generations=12, tol=0.01)
    batch, singles = batch_plan(q), single_plans(q)
    sts = batch.run(check_every=3)
    assert all(st["stop"] for st in sts)                                                  # run() returned once ALL flags were set
    for p in singles:
        p.run(check_every=3)
    assert_batch_equals_singles(batch, singles)
    assert sts[0]["generation"] == 2 and sts[0]["stop"] == nat.HM_DE_STOP_CONVERGED and sts[0]["std"] == 0.0
    for k in (1, 2):
        assert sts[k]["generation"] == 12 and sts[k]["stop"] == nat.HM_DE_STOP_MAX, sts[k]
    # a stopped problem is frozen: further generations of the batch move nothing of it, its rows included
    before = state_bytes(batch, 0)
    batch.launch()
    batch.launch()
    assert before == state_bytes(batch, 0)


@pytest.mark.parametrize("b", [12, 14])
def test_problems_stop_at_different_times(b):
    check_problems_stop_at_different_times("cpu", b)


def check_frozen_among_running(device, b):
    """The same freeze while the OTHER problems still run: problem 0 stops at generation 2 of 12, the batch goes on, and after every
    further launch problem 0's slices - trial rows, verdicts, trial energies - are the bytes they were when it stopped."""
    S, P = 16, 3
    pop = populations(2, S, P, 5)
    pop[0] = 0.5 * (TRUE[:P] + 1)
    q = make_batch(device, b, 2, (40, 40, 6), S, P, seeds=(7, 8), pop=pop, max_generations=12, tol=0.01)
    batch = batch_plan(q)
    for _ in range(3):
        batch.launch()
    sts = batch.read_status()
    assert sts[0]["stop"] == nat.HM_DE_STOP_CONVERGED and sts[1]["stop"] == 0
    before, other = state_bytes(batch, 0), state_bytes(batch, 1)
    for _ in range(3):
        batch.launch()
        assert state_bytes(batch, 0) == before
    assert state_bytes(batch, 1) != other and batch.read_status()[1]["generation"] == 5


@pytest.mark.parametrize("b", [12, 14])
def test_stopped_problem_is_frozen_while_others_run(b):
    check_frozen_among_running("cpu", b)


# ------------------------------------------------------------------------------------------------ 6: determinism
def run_state(q, check_every, graph=True, variant=None):
    plan = batch_plan(q, variant=variant)
    sts = plan.run(check_every, graph)
    return state_bytes(plan), sts


def check_determinism(device, graphs=(True,), b=12):
    q = make_batch(device, b, 3, (40, 40, 6), 8, 3, seeds=(7, 8, 9), max_generations=12)
    ref, sts = run_state(q, 8)
    assert all(st["generation"] == 12 and st["stop"] == nat.HM_DE_STOP_MAX for st in sts)
    for graph in graphs:
        for ce in (1, 3, 8):
            got, sts2 = run_state(q, ce, graph)
            assert got == ref and all(same_status(x, y) for x, y in zip(sts, sts2)), (graph, ce)
    for variant in (1, 2):                                                               # 1: the dynamic-LDS batched kernels, 2: the gather
        got, sts2 = run_state(q, 8, variant=variant)
        assert got == ref and all(same_status(x, y) for x, y in zip(sts, sts2)), variant
    # K = 1 is the single plan
    one = make_batch(device, b, 1, (40, 40, 6), 8, 3, seeds=(7,), max_generations=12)
    batch, singles = batch_plan(one, explicit_stack_of=False), single_plans(one)
    batch.run(8)
    singles[0].run(8)
    assert_batch_equals_singles(batch, singles)


def test_determinism_check_every_and_variants():
    check_determinism("cpu")


# ------------------------------------------------------------------------------------------------ 7: argument rules (no device needed)
EINVAL, ESHAPE, EUNSUP, EALIGN = nat.HM_EINVAL, nat.HM_ESHAPE, nat.HM_EUNSUPPORTED, nat.HM_EALIGN


@pytest.mark.parametrize("which", ["hip", "host"])
def test_abi_rejects_bad_arguments_without_a_device(which):
    """Every status of hm_de_generation_u16_batch in the header's order, from the argument checks: every refusal returns before any launch,
    so the device library answers on fake pointers (a launch attempt without a GPU would be HM_ELAUNCH)."""
    lib = nat.hip_lib if which == "hip" else nat.host_lib()
    fake = 0x7f0000000000
    t = (C.c_double * 5)(1, 2, 4, 8, 16)

    def call(K=3, S=16, P=3, N=5, null=(), dn_null=(), dn_odd=(), std=None, no_dn=False, no_seeds=False, **kw):
        ptrs = [None if i in null else fake + 4096 * i for i in range(11)]
        n = max(1, min(K, 64))
        dn = (C.c_void_p * n)(*[None if i in dn_null else fake + (1 << 24) * (i + 1) + (1 if i in dn_odd else 0) for i in range(n)])
        seeds = (C.c_int64 * n)(*range(n))
        sc = dict(n_pixels=100, lower=80, upper=4000, max_gen=10, m_lo=0.0, m_hi=1.95, cr=0.4, tol=0.01, e_lim=0.0, bits=12, variant=0,
                  ws=fake + (1 << 20))
        sc.update(kw)
        return lib.hm_de_generation_u16_batch(K, *ptrs, None if no_dn else dn, std, None if no_seeds else seeds, t, sc["n_pixels"], N,
                                              sc["lower"], sc["upper"], S, P, sc["max_gen"], sc["m_lo"], sc["m_hi"], sc["cr"], sc["tol"],
                                              sc["e_lim"], sc["bits"], sc["variant"], sc["ws"], None)
    # 1. hm_de_generation_batch's, in its order
    assert call(K=0) == EINVAL and call(K=-2) == EINVAL
    assert nat.HM_DE_MAX_PROBLEMS == 64 and call(K=65) == ESHAPE
    assert call(S=3) == EINVAL and call(P=0) == EINVAL and call(max_gen=-1) == EINVAL and call(n_pixels=-1) == EINVAL
    assert call(S=nat.HM_DE_MAX_POP + 1) == ESHAPE and call(P=nat.HM_DE_MAX_PARAMS + 1) == ESHAPE
    assert call(N=1) == ESHAPE and call(N=nat.HM_MAX_FRAMES + 1) == ESHAPE
    assert call(K=64, S=1024) == EUNSUP                                                  # 65 536 candidates: over the energy grid's limit
    assert call(K=63, S=1024, null=(0,)) == EINVAL                                       # 64 512 candidates pass that check (and meet the NULL one)
    assert call(cr=float("nan")) == EINVAL and call(m_hi=2.0) == EINVAL and call(m_lo=1.0, m_hi=0.5) == EINVAL
    assert call(tol=-1.0) == EINVAL and call(e_lim=float("nan")) == EINVAL
    for i in range(11):                                                                  # every state / model buffer
        assert call(null=(i,)) == EINVAL, i
    assert call(no_dn=True) == EINVAL and call(no_seeds=True) == EINVAL
    assert call(dn_null=(2,)) == EINVAL                                                  # one problem without a stack
    some = (C.c_void_p * 3)(fake + (1 << 30), None, fake + (1 << 31))
    assert call(std=some) == EINVAL                                                      # stds for all problems or for none
    # 2. hm_de_generation_u16's additions: depth, variant, limits of the depth (not the 8-bit limit rule), the LDS fit
    assert call(bits=8) == EINVAL and call(bits=17) == EINVAL
    assert call(variant=3) == EINVAL and call(variant=-1) == EINVAL
    assert call(lower=-1) == EINVAL and call(upper=4096) == EINVAL and call(bits=9, upper=512) == EINVAL
    assert call(bits=15, variant=1, upper=4000) == EUNSUP and call(bits=16, variant=1) == EUNSUP
    # 3. alignment of any stack
    assert call(dn_odd=(0,)) == EALIGN and call(dn_odd=(2,)) == EALIGN
    # an earlier rule wins
    assert call(K=65, S=3) == ESHAPE and call(K=0, bits=8) == EINVAL
    assert call(S=nat.HM_DE_MAX_POP + 1, bits=8) == ESHAPE and call(K=64, S=1024, bits=8) == EUNSUP
    assert call(bits=15, variant=1, upper=1 << 15) == EINVAL                             # the limit before the LDS fit
    assert call(bits=15, variant=1, dn_odd=(1,)) == EUNSUP and call(bits=8, dn_odd=(1,)) == EINVAL
    assert call(dn_null=(1,), dn_odd=(0,)) == EINVAL and call(dn_null=(1,), bits=8) == EINVAL      # a NULL entry before depth and alignment
    # the workspace is the 8-bit batch's function: 0 for every rejected shape, K times the single size otherwise
    for bad in ((100, 5, 16, 0), (100, 5, 16, 65), (100, 5, 3, 2), (100, 5, 1024, 64), (100, 5, 2048, 1)):
        assert lib.hm_de_batch_workspace_bytes(*bad) == 0, bad
    assert lib.hm_de_batch_workspace_bytes(784, 7, 128, 12) == 12 * lib.hm_de_workspace_bytes(784, 7, 128)
    if which == "hip":
        assert call(ws=None) == EINVAL                                                    # the device build's own, last
        assert call(ws=None, dn_odd=(0,)) == EALIGN
        single = lib.hm_de_workspace_bytes(784, 7, 128)
        assert single >= 16 * 128 and lib.hm_de_batch_workspace_bytes(784, 7, 128, 12) == 12 * single      # room for K S 16 verdict bytes
        if not torch.cuda.is_available():
            assert call() == nat.HM_ELAUNCH and call(bits=16, upper=65535) == nat.HM_ELAUNCH        # valid arguments meet no device
    # both libraries export the symbol; the change is additive
    assert "hm_de_generation_u16_batch" in nat.EXPORTED_SYMBOLS and callable(lib.hm_de_generation_u16_batch)
    assert nat.HM_ABI_VERSION == 2 and lib.hm_version() == 2


# ------------------------------------------------------------------------------------------------ 8: the Python layer
def check_plan_refusals(device):
    q = make_batch(device, 12, 2, (12, 12, 4), 8, 3, seeds=(1, 2))
    eng, (lo, hi) = eng_of(q), limits(12)

    def build(lower=lo, upper=hi, b=12, variant=0, **over):
        a = dict(q, **over)
        return eng.DEBatchPlanU16(a["stacks"], a["stds"], a["t"], a["means"], a["pcas"], -1.0, 1.0, a["pop"], lower, upper, a["seeds"], 10,
                                  stack_of=over.get("stack_of"), bit_depth=b, variant=variant)
    p = build()
    assert p.K == 2 and p.bit_depth == 12 and tuple(p.icrf.shape) == (2, 8, 4096) and tuple(p.status.shape) == (2, nat.HM_DE_STATUS_WORDS)
    assert build(b=[12, 12]).bit_depth == 12
    u8 = torch.zeros((12, 12, 4), dtype=torch.uint8, device=device)
    with pytest.raises(TypeError, match="DEBatchPlan"):
        build(stacks=[q["stacks"][0], u8])                                               # uint8 DNs: the 8-bit plan's
    with pytest.raises(TypeError, match="uint16"):
        build(stacks=[q["stacks"][0], q["stacks"][1].to(torch.float64)])
    other = torch.zeros((12, 10, 4), dtype=torch.int16, device=device).view(torch.uint16)
    with pytest.raises(ValueError, match="one shape"):
        build(stacks=[q["stacks"][0], other])
    with pytest.raises(ValueError, match="one bit depth"):
        build(b=[12, 14])
    with pytest.raises(ValueError, match="bit_depth"):
        build(b=None)
    for bad in (8, 17, 12.0):
        with pytest.raises(ValueError, match="bit_depth"):
            build(b=bad)
    with pytest.raises(ValueError, match=r"every mean ICRF must have 4096 entries and every PCA basis must be \(4096, 3\)"):
        build(means=[q["means"][0], q["means"][1][:256]])                                # a wrong number of table rows
    with pytest.raises(ValueError, match=r"every mean ICRF must have 2048 entries"):
        build(b=11, upper=2000)
    with pytest.raises(ValueError, match="PCA basis"):
        build(pcas=[q["pcas"][0], q["pcas"][1][:, :2]])
    for lower, upper in ((-1, 4000), (80, 4096)):
        with pytest.raises(ValueError, match="lower and upper"):
            build(lower=lower, upper=upper)
    with pytest.raises(ValueError, match="variant"):
        build(variant=3)
    with pytest.raises(ValueError, match="1 to 64 problems"):
        build(pop=np.full((65, 8, 3), 0.5), stack_of=[0] * 65, seeds=list(range(65)), means=[q["means"][0]] * 65, pcas=[q["pcas"][0]] * 65)
    with pytest.raises(ValueError, match="stack_of"):
        build(stack_of=[0, 2])
    with pytest.raises(ValueError, match="stack_of"):
        build(stacks=q["stacks"][:1])                                                    # one stack, two problems, no stack_of
    assert build(stacks=q["stacks"][:1], stack_of=[0, 0]).K == 2
    sd = torch.full((12, 12, 4), 0.01, dtype=torch.float64, device=device)
    with pytest.raises(ValueError, match="every stack of a batch or for none"):
        build(stds=[sd, None])
    assert build(stds=[sd, sd]).std is not None
    with pytest.raises(ValueError, match="one entry per problem"):
        build(seeds=[1])
    with pytest.raises(ValueError, match=r"\(K, S, P\)"):
        build(pop=q["pop"][0])
    with pytest.raises(ValueError):
        p.run(0)
    # variant 1 where the row does not fit LDS: the entry's status, before any launch
    q16 = make_batch(device, 16, 2, (12, 12, 4), 8, 3, seeds=(1, 2))
    plan = batch_plan(q16, variant=1)
    with pytest.raises(NotImplementedError, match="hm_de_generation_u16_batch"):
        plan.launch()
    assert all(st["evaluations"] == 0 for st in plan.read_status())
    # the raising paths of the 8-bit names still raise on uint16 stacks
    pr = du.make_problem(device, 12)
    with pytest.raises(TypeError, match="image_value_stack must be uint8 digital numbers"):
        eng.DEPlan(pr["stack"], None, pr["t"], pr["mean"], pr["pca"], -1.0, 1.0, np.full((16, 3), 0.5), 5, 250, 1, 10)
    with pytest.raises(TypeError, match="image_value_stack must be uint8 digital numbers"):
        eng.DEBatchPlan(q["stacks"], None, q["t"], q["means"], q["pcas"], -1.0, 1.0, q["pop"], 5, 250, q["seeds"], 10)
    for kw in (dict(solver="device"), dict(solver="device", restarts=2)):
        with pytest.raises(NotImplementedError, match='solver="scipy"'):
            ic.solve_channel(pr["mean"], pr["pca"], pr["stack"], None, pr["t"], -1.0, 1.0, bit_depth=12, **kw)
    for kw in (dict(solver="device"), dict(solver="device", batched=True), dict(solver="device", restarts=2)):
        with pytest.raises(NotImplementedError, match='solver="scipy"'):
            ic.calibration([pr["mean"]], [pr["pca"]], pr["stacks"], [None], pr["t"], -1.0, 1.0, bit_depth=12, **kw)


def test_plan_refusals():
    check_plan_refusals("cpu")
    q = make_batch("cpu", 12, 2, (12, 12, 4), 8, 3, seeds=(1, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                           # host tensors outside host_mode(): the HIP backend refuses
        engine.DEBatchPlanU16(q["stacks"], None, q["t"], q["means"], q["pcas"], -1.0, 1.0, q["pop"], 80, 4000, q["seeds"], 10, bit_depth=12)


def channel_problem(device, b=10):
    """Three different 24 x 24 x 5 channel stacks at depth b with their cameras."""
    cams = [camera(k, 3, b) for k in range(3)]
    stacks, t = [], None
    for c, (mean, pca) in enumerate(cams):
        dn, t = synthetic_stack(device, du.SHAPE, 300 + c, mean, pca, b)
        stacks.append(dn)
    return [c[0] for c in cams], [c[1] for c in cams], stacks, t


def check_calibration_batched(device, lib, b=10):
    means, pcas, stacks, t = channel_problem(device, b)
    args = (means, pcas, stacks, [None] * 3, t, -1.0, 1.0, b)
    for restarts in (1, 2):
        calls = (lib.calls["hm_de_generation_u16_batch"], lib.calls["hm_de_generation_u16"])
        table_b, e_b = ic.calibration_u16(*args, max_iterations=6, restarts=restarts, batched=True)
        assert lib.calls["hm_de_generation_u16_batch"] > calls[0] and lib.calls["hm_de_generation_u16"] == calls[1]
        table_s, e_s = ic.calibration_u16(*args, max_iterations=6, restarts=restarts)
        assert lib.calls["hm_de_generation_u16"] > calls[1]
        np.testing.assert_array_equal(table_b, table_s)
        np.testing.assert_array_equal(e_b, e_s)
        assert table_b.shape == (2 ** b, 3) and np.all(np.isfinite(e_b)) and len(set(e_b.tolist())) == 3
    with pytest.raises(ValueError, match="PCA components"):
        ic.calibration_u16(means, [pcas[0], pcas[1], pcas[2][:, :2]], stacks, [None] * 3, t, -1.0, 1.0, b, batched=True)
    with pytest.raises(ValueError, match="one shape"):
        ic.calibration_u16(means, pcas, [stacks[0], stacks[1], stacks[2][:20].contiguous()], [None] * 3, t, -1.0, 1.0, b, batched=True)
    with pytest.raises(ValueError, match="restarts"):
        ic.calibration_u16(*args, restarts=0, batched=True)


def test_calibration_batched_equals_sequential():
    check_calibration_batched("cpu", nat.host_lib())


def check_restarts(device, b=10):
    means, pcas, stacks, t = channel_problem(device, b)
    args = (means[0], pcas[0], stacks[0], None, t, -1.0, 1.0, b)
    singles = [ic.solve_channel_u16(*args, seed=ic.restart_seed(7, r), max_iterations=6) for r in range(3)]
    assert len({s[1] for s in singles}) == 3
    seq = ic.solve_channel_u16(*args, seed=7, max_iterations=6, restarts=3)
    icrf, e, n_it = ic.solve_channel_u16(*args, seed=7, max_iterations=6, restarts=3, batched=True)
    np.testing.assert_array_equal(icrf, seq[0])
    assert (e, n_it) == seq[1:] and all(e <= s[1] for s in singles)                      # never worse than any of its seeds alone
    one = ic.solve_channel_u16(*args, seed=7, max_iterations=6, batched=True)            # K = 1
    assert np.array_equal(one[0], singles[0][0]) and one[1:] == singles[0][1:]
    with pytest.raises(ValueError, match="restarts"):
        ic.solve_channel_u16(*args, seed=7, restarts=0, batched=True)


def test_restarts_batched_equal_the_sequential_restarts():
    check_restarts("cpu")


def test_more_than_64_problems_go_in_consecutive_batches(monkeypatch):
    """calibration_u16(batched=True) cuts C x R problems into batches of at most HM_DE_MAX_PROBLEMS, in order, and keeps the best restart
    of every channel (the batches are stubbed: the cut is what is checked)."""
    seen = []

    def stub(means, pcas, stacks, std_stacks, stack_of, seeds, *args, **kw):
        seen.append((list(stack_of), list(seeds), kw["bit_depth"]))
        return [(np.linspace(0, 1, 1024) * (1 + 1e-3 * c), float(sd % 1000), 1) for c, sd in zip(stack_of, seeds)]
    monkeypatch.setattr(ic, "_solve_batch", stub)
    Cn, R = 3, 30
    table, e = ic.calibration_u16([np.zeros(1024)] * Cn, [np.zeros((1024, 2))] * Cn, [None] * Cn, [None] * Cn, None, -1.0, 1.0, 10, rng_seed=7,
                                  restarts=R, batched=True)
    assert [len(s[0]) for s in seen] == [64, 26] and all(s[2] == 10 for s in seen)
    assert sum((s[0] for s in seen), []) == [c for c in range(Cn) for _ in range(R)]
    assert sum((s[1] for s in seen), []) == [ic.restart_seed(7 + c, r) for c in range(Cn) for r in range(R)]
    np.testing.assert_array_equal(e, [min(float(ic.restart_seed(7 + c, r) % 1000) for r in range(R)) for c in range(Cn)])
    assert table.shape == (1024, Cn)


def test_new_arguments_default_to_the_old_behaviour():
    import inspect
    assert inspect.signature(ic.solve_channel_u16).parameters["batched"].default is False
    assert inspect.signature(ic.calibration_u16).parameters["batched"].default is False
    assert inspect.signature(ic.calibration_u16).parameters["restarts"].default == 1
    par = inspect.signature(ic.solve_channel_u16).parameters
    assert ic._device_defaults(ic.solve_channel_u16) == {k: par[k].default for k in ("check_every", "graph", "tol")}


def test_host_batch_never_reaches_the_hip_library():
    q = make_batch("cpu", 10, 2, (12, 12, 4), 8, 3, seeds=(1, 2), max_generations=4)
    hip, h = nat.hip_lib.calls, nat.host_lib().calls
    before = (hip["hm_de_generation_u16_batch"], hip["hm_de_generation_u16"], hip["hm_linearity_energy_u16"], h["hm_de_generation_u16_batch"])
    batch_plan(q).run(2)
    assert (hip["hm_de_generation_u16_batch"], hip["hm_de_generation_u16"], hip["hm_linearity_energy_u16"]) == before[:3]
    assert h["hm_de_generation_u16_batch"] >= before[3] + 5
