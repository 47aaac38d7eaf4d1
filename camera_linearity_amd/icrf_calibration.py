"""ICRF calibration by exposure linearity - mirror of modules/ICRF_calibration_exposure.py on the HIP backend.

The reference minimises, per channel, an energy function with SciPy's differential-evolution solver; every
evaluation maps the (X, Y, N) channel stack through a candidate ICRF and reduces an (X, Y, N, N) array of
pairwise relative differences on the host (ICRF_calibration_exposure.py:66-201), one candidate at a time.
Here the stack stays on the device and `hm_linearity_energy` evaluates a whole POPULATION of candidates in one
launch (grid = pixel chunks x frame pairs x candidates). By default (`solver="scipy"`) the solver itself stays SciPy's,
on the host, driven through its `vectorized=True` interface (one launch per generation) or, for the reference's exact
update order, one candidate per call; the candidate ICRF (mean + PCA product, shift, range / monotonicity rejection:
:22-45,:166-179) is then 256 numbers per candidate formed on the host with NumPy, like the reference.

`solver="device"` runs the whole generation - mutation, crossover, candidate ICRFs and their verdicts, energy, selection,
convergence statistics - where the stack lives (hm_de_generation, engine.DEPlan): the same strategy and settings, restated
with counter-based random numbers (include/hdrmerge.h), started from SciPy's own Sobol population. Several such problems of one shape -
the channels of a calibration (`calibration(..., batched=True)`), restarts of a channel with other seeds (`restarts=R`), or both - run
in ONE plan (hm_de_generation_batch, engine.DEBatchPlan): one set of launches per generation for all of them, each problem evolving bit
for bit as it would alone.

A 9- to 16-bit camera's torch.uint16 stacks have the device solver under names of their own, `solve_channel_u16` and `calibration_u16`
(hm_de_generation_u16, engine.DEPlanU16: rows of 2**bit_depth entries), and with `batched=True` the restarts of a channel or all channels
and restarts of a calibration in ONE plan (hm_de_generation_u16_batch, engine.DEBatchPlanU16); `solve_channel` / `calibration` with a
`bit_depth` stay on SciPy's solver.
"""
from __future__ import annotations

import inspect
from typing import Optional, Sequence

import numpy as np
import torch
from scipy.optimize._differentialevolution import DifferentialEvolutionSolver   # same access as the reference (:7)

from . import _native as nat
from . import engine
from . import settings as gs


def _inverse_camera_response_function(mean_ICRF, PCA_array, PCA_params, use_mean_ICRF):
    """:22-45. PCA_params may be one vector (n_params,) or a batch (n_candidates, n_params); returns (n,) or
    (n_candidates, n) with n the rows of the PCA basis: 256, or 2**bit_depth for a deeper camera (the power-law base takes its grid from
    there, not from settings.BITS)."""
    p = np.asarray(PCA_params, dtype=np.float64)
    single = p.ndim == 1
    p = np.atleast_2d(p)
    if not use_mean_ICRF:
        base = np.linspace(0, 1, np.shape(PCA_array)[0])[None, :] ** p[:, :1]
        out = np.stack([base[b] + np.matmul(PCA_array, p[b, 1:]) for b in range(p.shape[0])])
    else:
        out = np.stack([mean_ICRF + np.matmul(PCA_array, p[b]) for b in range(p.shape[0])])
    return out[0] if single else out


def candidate_icrfs(PCA_params, mean_ICRF, PCA_array, use_mean_ICRF=True):
    """Candidate ICRFs as the energy function sees them (:165-179): shifted so that ICRF[-1] = 1 and ICRF[0] = 0, and the
    per-candidate verdict of the range and strict-monotonicity tests. -> (icrfs (B, n), valid (B,) bool), n the rows of the mean ICRF / PCA
    basis (256, or 2**bit_depth)."""
    icrfs = np.atleast_2d(_inverse_camera_response_function(mean_ICRF, PCA_array, PCA_params, use_mean_ICRF)).copy()
    icrfs += (1 - icrfs[:, -1])[:, None]                                         # :166
    icrfs[:, 0] = 0                                                              # :167
    valid = ~((icrfs.max(axis=1) > 1) | (icrfs.min(axis=1) < 0))                 # :173-175
    valid &= np.all(icrfs[:, 1:] > icrfs[:, :-1], axis=1)                        # :177-179
    return icrfs, valid


def analyze_linearity(image_value_stack: torch.Tensor, image_std_stack: Optional[torch.Tensor], ICRF_ch, lower: int, upper: int,
                      use_relative: bool, exposure_values, bit_depth: Optional[int] = None):
    """:66-145 for a uint8 DN stack seen through one ICRF: the N(N-1)/2 pair results (device tensor) in
    np.triu_indices(N, 1) order. `lower` / `upper` are DN limits (the energy function maps them through the ICRF, :181-182).
    bit_depth=b (9..16): a torch.uint16 stack, an ICRF of 2**b entries, limits that are DNs of that depth."""
    _, pairs = _engine_for(image_value_stack).linearity_energy(image_value_stack, image_std_stack, _host(exposure_values),
                                                               np.asarray(ICRF_ch)[None], lower, upper, None, use_relative, return_pairs=True,
                                                               bit_depth=bit_depth)
    return pairs[0]


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def _engine_for(stack: torch.Tensor):
    """The HIP library for a device-resident stack; the host build of the same ABI for a host stack (initialize_channel_image_stacks(...,
    device="cpu")). The reference makes this choice once per calibration - `calibration(..., use_cupy)` switches the module's array
    library (modules/ICRF_calibration_exposure.py:17, :317-319) and the stacks are created in it; here the choice is the `device` the
    caller gives initialize_channel_image_stacks (default: the current GPU - it raises without one) and every later call follows the
    stacks' placement. Never a fallback: a device stack never computes on the host."""
    if not isinstance(stack, torch.Tensor) or stack.is_cuda:        # (anything but a tensor: engine raises the TypeError)
        return engine
    from .measurand import _HOST_ENGINE
    return _HOST_ENGINE


def energy_function_batch(PCA_params, mean_ICRF, PCA_array, image_value_stack, image_std_stack, lower, upper, use_mean,
                          exposure_values, bit_depth: Optional[int] = None) -> np.ndarray:
    """Energies of a batch of candidates. PCA_params: (n_candidates, n_params). One device launch.
    bit_depth=b (9..16): a torch.uint16 stack, mean ICRF and PCA basis of 2**b rows."""
    icrfs, valid = candidate_icrfs(PCA_params, mean_ICRF, PCA_array, use_mean)
    if not valid.any():
        return np.full(len(valid), np.inf)
    e = _engine_for(image_value_stack).linearity_energy(image_value_stack, image_std_stack, _host(exposure_values), icrfs, int(lower), int(upper),
                                valid, True, bit_depth=bit_depth)
    return e.cpu().numpy()


def _energy_function(PCA_params, mean_ICRF, PCA_array, image_value_stack, image_std_stack, lower, upper, use_mean,
                     exposure_values, bit_depth: Optional[int] = None):
    """:148-201, the reference's signature: one candidate -> float. With a (n_params, S) array (SciPy's
    `vectorized=True` calling convention) -> (S,) energies from one launch. `bit_depth` trails, so SciPy's `args` tuple carries it."""
    p = np.asarray(PCA_params, dtype=np.float64)
    if p.ndim == 2:
        return energy_function_batch(p.T, mean_ICRF, PCA_array, image_value_stack, image_std_stack, lower, upper, use_mean,
                                     exposure_values, bit_depth)
    return float(energy_function_batch(p[None], mean_ICRF, PCA_array, image_value_stack, image_std_stack, lower, upper, use_mean,
                                       exposure_values, bit_depth)[0])


def interpolate_ICRF(ICRF_array, datapoints: Optional[int] = None, bits: Optional[int] = None):
    """:204-216: resample (DATAPOINTS, C) to (BITS, C) by linear interpolation when the sizes differ. `bits`: the rows to resample to
    instead of settings.BITS (2**bit_depth for a deeper camera)."""
    ICRF_array = np.asarray(ICRF_array, dtype=np.float64)
    datapoints = ICRF_array.shape[0] if datapoints is None else datapoints
    bits = gs.BITS if bits is None else int(bits)
    if bits == datapoints:
        return ICRF_array
    x_new = np.linspace(0, 1, num=bits)
    x_old = np.linspace(0, 1, num=datapoints)
    out = np.zeros((bits, ICRF_array.shape[1]), dtype=float)
    for c in range(ICRF_array.shape[1]):
        out[:, c] = np.interp(x_new, x_old, ICRF_array[:, c])
    return out


def initialize_channel_image_stacks(frames: Sequence, exposures: Sequence[float], stds: Optional[Sequence] = None,
                                    data_spacing=150, device=None, bit_depth: Optional[int] = None):
    """:219-284 for frames already in memory (uint8 (H, W, C) arrays / tensors): sort by exposure, thin the pixels with
    `data_spacing` (int or (x_step, y_step); plain strided selection) and stack every channel to (X, Y, N).
    -> (channel value stacks [C x uint8 (X, Y, N) device tensors], channel std stacks or [None]*C, exposures ndarray).
    bit_depth=b (9..16): uint16 frames of a b-bit camera, kept as torch.uint16 stacks for calibration(..., bit_depth=b). uint16 frames
    without it raise ValueError (cast to uint8 they would wrap)."""
    u16 = [(f.dtype == torch.uint16) if isinstance(f, torch.Tensor) else (np.asarray(f).dtype == np.uint16) for f in frames]
    if bit_depth is not None:
        engine._check_bit_depth(bit_depth)
        if not all(u16):
            raise ValueError("bit_depth is for uint16 frames")
    elif any(u16):
        raise ValueError("uint16 frames need bit_depth (9..16): as uint8 stacks their DNs would wrap")
    dn_dtype = torch.uint8 if bit_depth is None else torch.uint16
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    x_step, y_step = data_spacing if isinstance(data_spacing, tuple) else (data_spacing, data_spacing)
    order = np.argsort(np.asarray(exposures, dtype=np.float64), kind="stable")
    t = np.asarray(exposures, dtype=np.float64)[order]

    def thin(img, dtype):
        a = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
        return a[::x_step, ::y_step].to(device=device, dtype=dtype)

    # (uint16 frames are stacked as their int16 bit patterns: torch implements few operations for unsigned 16-bit tensors)
    as_stacked = (lambda x: x) if bit_depth is None else (lambda x: x.view(torch.int16))
    vals = torch.stack([as_stacked(thin(frames[i], dn_dtype)) for i in order], dim=-1)            # (X, Y, C, N)
    value_stacks = [vals[:, :, c, :].contiguous().view(dn_dtype) for c in range(vals.shape[2])]
    if stds is not None:
        sds = torch.stack([thin(stds[i], torch.float64) for i in order], dim=-1)
        std_stacks = [sds[:, :, c, :].contiguous() for c in range(sds.shape[2])]
    else:
        std_stacks = [None] * vals.shape[2]
    return value_stacks, std_stacks, t


RESTART_SEED_STRIDE = 1_000_003


def restart_seed(seed: int, restart: int) -> int:
    """The seed of restart r of a solve seeded with `seed`: seed + 1 000 003 r. Restart 0 is the solve itself; the stride keeps the
    restarts of channel c (seeded rng_seed + c by calibration()) away from the seeds of the other channels."""
    return int(seed) + RESTART_SEED_STRIDE * int(restart)


def _seed_keyword(seed) -> dict:
    # the reference passes seed= (SciPy 1.14, its Pipfile.lock); SciPy >= 1.15 renamed the argument to rng=
    return {"rng" if "rng" in inspect.signature(DifferentialEvolutionSolver.__init__).parameters else "seed": seed}


def _pca_limits(n_components: int, lower_PCA_limit: float, upper_PCA_limit: float):
    """Search limits and start point of a mean-ICRF solve (:313-315)."""
    return [[lower_PCA_limit, upper_PCA_limit] for _ in range(n_components)], [0] * n_components


def _initial_population(limits, x0, args, tol, popsize, extra) -> np.ndarray:
    """SciPy's own initial population (Sobol, the seed in `extra`), read without iterating: both solvers start from the same S x P points."""
    with DifferentialEvolutionSolver(_energy_function, limits, args=args, strategy="currenttobest1bin", tol=tol, x0=x0,
                                     mutation=(0, 1.95), recombination=0.4, init="sobol", popsize=popsize, **extra) as start:
        return np.array(start.population, dtype=np.float64)


def _solve_batch(means, pcas, stacks, std_stacks, stack_of, seeds, exposure_values, lower_PCA_limit, upper_PCA_limit, data_limits,
                 energy_limit, max_iterations, popsize, check_every, graph, tol, bit_depth=None, variant=0):
    """K device solves of one shape in one engine.DEBatchPlan: problem k on stacks[stack_of[k]] with means[k], pcas[k], seeds[k] and
    SciPy's Sobol population for seeds[k]. -> [(icrf, energy, iterations)] * K, each what solve_channel(solver="device") returns for it.
    bit_depth=b: torch.uint16 stacks of a b-bit camera in one engine.DEBatchPlanU16 (`variant`: the placement of a candidate's row), each
    triple what solve_channel_u16 returns for it."""
    K = len(seeds)
    pcas = [np.asarray(b, dtype=np.float64) for b in pcas]
    n_params = {b.shape[1] for b in pcas}
    if len(n_params) != 1:
        raise ValueError(f"a batched solve needs the same number of PCA components for every problem, got {[b.shape[1] for b in pcas]}")
    shapes = {tuple(s.shape) for s in stacks}
    if len(shapes) != 1:
        raise ValueError(f"a batched solve needs channel stacks of one shape, got {[tuple(s.shape) for s in stacks]}")
    limits, x0 = _pca_limits(n_params.pop(), lower_PCA_limit, upper_PCA_limit)
    for sd in seeds:
        if not isinstance(sd, (int, np.integer)):
            raise TypeError('solver="device" needs an integer seed')
    pops = []
    for k in range(K):
        c = stack_of[k]
        args = (means[k], pcas[k], stacks[c], std_stacks[c], data_limits[0], data_limits[1], True, exposure_values) + \
            (() if bit_depth is None else (bit_depth,))
        pops.append(_initial_population(limits, x0, args, tol, popsize, dict(vectorized=True, updating="deferred", **_seed_keyword(seeds[k]))))
    lo, hi = np.asarray(limits, dtype=np.float64).T
    eng = _engine_for(stacks[0])
    plan_args = (stacks, std_stacks, _host(exposure_values), means, pcas, lo, hi, np.stack(pops), data_limits[0], data_limits[1],
                 [int(sd) for sd in seeds], 2 * int(max_iterations), (0.0, 1.95), 0.4, tol, energy_limit)
    if bit_depth is None:
        plan = eng.DEBatchPlan(*plan_args, stack_of=stack_of)
    else:
        plan = eng.DEBatchPlanU16(*plan_args, stack_of=stack_of, bit_depth=bit_depth, variant=variant)
    sts = plan.run(check_every, graph)
    best = plan.population[torch.arange(K), torch.as_tensor([st["best_index"] for st in sts])].cpu().numpy()      # one copy for the K members
    return [(_inverse_camera_response_function(means[k], pcas[k], lo + best[k] * (hi - lo), True), sts[k]["best_energy"],
             sts[k]["generation"] // 2) for k in range(K)]


def _best_restart(results):
    """The restart with the lowest final energy; ties go to the lowest restart index."""
    return min(enumerate(results), key=lambda ir: (ir[1][1], ir[0]))[1]


def _device_defaults(solve=None):
    """solve_channel's own defaults of check_every, graph and tol: what calibration()'s sequential path inherits by not passing them,
    handed to the batched path from the same place, so the two stay array-equal if a default moves. `solve`: another solve function to
    read them from (calibration_u16: solve_channel_u16)."""
    import inspect
    par = inspect.signature(solve_channel if solve is None else solve).parameters
    return {name: par[name].default for name in ("check_every", "graph", "tol")}


def _scipy_only(bit_depth, solver, batched, restarts):
    """solve_channel / calibration with a bit depth run on SciPy's solver: their device solver forms candidate rows of 256 entries. The
    device solver for uint16 stacks has entries of its own, solve_channel_u16 and calibration_u16."""
    engine._check_bit_depth(bit_depth)
    if solver == "device" or batched or restarts > 1:
        raise NotImplementedError('bit_depth needs solver="scipy" without batched=True or restarts > 1 here: this device solver forms '
                                  'candidate ICRFs of 256 entries. The device solver for uint16 stacks is solve_channel_u16 / '
                                  'calibration_u16 (one problem per plan)')


def solve_channel(mean_ICRF_array, PCA_array, image_value_stack, image_std_stack, exposure_values,
                  lower_PCA_limit: float, upper_PCA_limit: float, use_mean_ICRF: bool = True,
                  data_limits=(gs.LOWER_LIN_LIM, gs.UPPER_LIN_LIM), energy_limit: float = 0.0, seed=7,
                  max_iterations: int = 1000, vectorized: bool = True, popsize: int = 15, channel: int = 0, verbose: bool = False,
                  solver: str = "scipy", check_every: int = 8, graph: bool = True, tol: float = 0.01, restarts: int = 1,
                  bit_depth: Optional[int] = None):
    """The per-channel solve of calibration() (:329-369): SciPy's DifferentialEvolutionSolver with the reference's
    settings. vectorized=True evaluates each generation's population in ONE launch (SciPy then uses deferred updating);
    vectorized=False keeps the reference's immediate updating and evaluates one candidate per launch.
    solver="device": the generations run on the stack's backend (engine.DEPlan; deferred updating, SciPy's initial population, the
    library's own random numbers), `check_every` generations per status read, recorded as a hipGraph unless graph=False; `vectorized`
    does not apply. An iteration is two generations, as in the reference loop. `tol` is the solver's relative convergence tolerance
    (the reference's 0.01) for either solver.
    restarts=R > 1 (solver="device" only): R solves of the same channel from other seeds - restart r uses restart_seed(seed, r) =
    seed + 1 000 003 r, so restart 0 is the restarts=1 solve, and starts from SciPy's Sobol population for that seed - advanced together
    in one engine.DEBatchPlan; the triple of the restart with the lowest final energy is returned (ties: the lowest r).
    bit_depth=b (9..16, solver="scipy" only; the device solver for such a stack is solve_channel_u16): a torch.uint16 stack of a b-bit
    camera, mean ICRF and PCA basis of 2**b rows. `data_limits`
    are DNs of the stack's depth and are not rescaled: the defaults are 8-bit DNs and wrong for any other depth.
    -> (ICRF of the channel (256,) - (2**b,) with bit_depth -, final energy, iterations)."""
    if solver not in ("scipy", "device"):
        raise ValueError(f"solver must be 'scipy' or 'device', got {solver!r}")
    restarts = int(restarts)
    if restarts < 1:
        raise ValueError(f"restarts must be >= 1, got {restarts}")
    if bit_depth is not None:
        _scipy_only(bit_depth, solver, False, restarts)
    if restarts > 1 and solver != "device":
        raise ValueError('restarts > 1 needs solver="device": the restarts run as one batch on the stack\'s backend')
    if solver == "device" and not use_mean_ICRF:
        raise NotImplementedError('solver="device" forms candidates from a mean ICRF only; the power-law base (use_mean_ICRF=False) needs '
                                  'solver="scipy"')
    PCA_array = np.asarray(PCA_array, dtype=np.float64)
    n_params = PCA_array.shape[1] + (0 if use_mean_ICRF else 1)
    limits, x0 = [], []
    if not use_mean_ICRF:
        limits.append([1, 8])                                                    # :309-311
        x0.append(3)
    for _ in range(PCA_array.shape[1]):
        limits.append([lower_PCA_limit, upper_PCA_limit])                        # :313-315
        x0.append(0)
    assert len(limits) == n_params
    args = (mean_ICRF_array, PCA_array, image_value_stack, image_std_stack, data_limits[0], data_limits[1], use_mean_ICRF,
            exposure_values) + (() if bit_depth is None else (bit_depth,))
    extra = dict(vectorized=True, updating="deferred") if vectorized else {}
    extra.update(_seed_keyword(seed))
    if solver == "device" and restarts > 1:
        if not isinstance(seed, (int, np.integer)):
            raise TypeError('solver="device" needs an integer seed')
        return _best_restart(_solve_batch([mean_ICRF_array] * restarts, [PCA_array] * restarts, [image_value_stack], [image_std_stack],
                                          [0] * restarts, [restart_seed(seed, r) for r in range(restarts)], exposure_values,
                                          lower_PCA_limit, upper_PCA_limit, data_limits, energy_limit, max_iterations, popsize,
                                          check_every, graph, tol))
    if solver == "device":
        population = _initial_population(limits, x0, args, tol, popsize, extra)
        if not isinstance(seed, (int, np.integer)):
            raise TypeError('solver="device" needs an integer seed')
        lo, hi = np.asarray(limits, dtype=np.float64).T
        plan = _engine_for(image_value_stack).DEPlan(image_value_stack, image_std_stack, _host(exposure_values), mean_ICRF_array, PCA_array,
                                                     lo, hi, population, data_limits[0], data_limits[1], int(seed), 2 * int(max_iterations),
                                                     (0.0, 1.95), 0.4, tol, energy_limit)
        st = plan.run(check_every, graph)
        u = plan.population[st["best_index"]].cpu().numpy()
        icrf = _inverse_camera_response_function(mean_ICRF_array, PCA_array, lo + u * (hi - lo), use_mean_ICRF)
        return icrf, st["best_energy"], st["generation"] // 2
    number_of_iterations = 0
    func_value = np.inf
    with DifferentialEvolutionSolver(_energy_function, limits, args=args, strategy="currenttobest1bin", tol=tol, x0=x0,
                                     mutation=(0, 1.95), recombination=0.4, init="sobol", popsize=popsize,
                                     **extra) as solver:                          # :344-347
        for step in solver:
            number_of_iterations += 1
            try:
                step = next(solver)          # as written (:351): every pass of the loop advances two generations
            except StopIteration:
                pass
            func_value = step[1]
            if verbose and number_of_iterations % 20 == 0:
                print(f"Channel {channel} value: {func_value} on step {number_of_iterations}")
            if solver.converged() or number_of_iterations == max_iterations or func_value < energy_limit:   # :356
                break
        result = solver.x
    icrf = _inverse_camera_response_function(mean_ICRF_array, PCA_array, result, use_mean_ICRF)
    return icrf, float(func_value), number_of_iterations


def _data_limits_u16(data_limits, bit_depth: int):
    """The DN limits of a uint16 solve: as given (DNs of the stack's depth), or the 8-bit defaults shifted to that depth."""
    if data_limits is None:
        return gs.LOWER_LIN_LIM << (bit_depth - 8), gs.UPPER_LIN_LIM << (bit_depth - 8)
    return int(data_limits[0]), int(data_limits[1])


def solve_channel_u16(mean_ICRF_array, PCA_array, image_value_stack, image_std_stack, exposure_values, lower_PCA_limit: float,
                      upper_PCA_limit: float, bit_depth: int, data_limits=None, energy_limit: float = 0.0, seed: int = 7,
                      max_iterations: int = 1000, popsize: int = 15, check_every: int = 8, graph: bool = True, tol: float = 0.01,
                      restarts: int = 1, variant: int = 0, batched: bool = False):
    """solve_channel(solver="device") for one channel of a 9- to 16-bit camera: a torch.uint16 stack, a mean ICRF of 2**bit_depth entries
    and a PCA basis of (2**bit_depth, P). The generations run on the stack's backend (engine.DEPlanU16, hm_de_generation_u16) from SciPy's
    Sobol population for `seed`, with the 8-bit device solver's strategy, settings and random numbers. `data_limits` are DNs of the stack's
    depth (default: the 8-bit limits shifted to it); `variant` places a candidate's row for the energy stage (engine.linearity_energy) and
    does not change the result. restarts=R > 1: R plans one after another, restart r seeded restart_seed(seed, r) - restart 0 is the
    restarts=1 solve -, the one with the lowest final energy returned (ties: the lowest r). batched=True runs the R restarts as ONE
    engine.DEBatchPlanU16 on the shared stack (hm_de_generation_u16_batch: one set of launches per generation for all of them, each
    evolving bit for bit as it would alone): the same return value, as arrays and floats.
    -> (ICRF of the channel (2**bit_depth,), final energy, iterations)."""
    bit_depth = engine._check_bit_depth(bit_depth)
    restarts = int(restarts)
    if restarts < 1:
        raise ValueError(f"restarts must be >= 1, got {restarts}")
    if not isinstance(seed, (int, np.integer)):
        raise TypeError("solve_channel_u16 needs an integer seed")
    PCA_array = np.asarray(PCA_array, dtype=np.float64)
    data_limits = _data_limits_u16(data_limits, bit_depth)
    if batched:
        return _best_restart(_solve_batch([mean_ICRF_array] * restarts, [PCA_array] * restarts, [image_value_stack], [image_std_stack],
                                          [0] * restarts, [restart_seed(seed, r) for r in range(restarts)], exposure_values,
                                          lower_PCA_limit, upper_PCA_limit, data_limits, energy_limit, max_iterations, popsize,
                                          check_every, graph, tol, bit_depth=bit_depth, variant=variant))
    limits, x0 = _pca_limits(PCA_array.shape[1], lower_PCA_limit, upper_PCA_limit)
    lo, hi = np.asarray(limits, dtype=np.float64).T
    args = (mean_ICRF_array, PCA_array, image_value_stack, image_std_stack, data_limits[0], data_limits[1], True, exposure_values, bit_depth)
    results = []
    for r in range(restarts):
        sd = restart_seed(seed, r)
        population = _initial_population(limits, x0, args, tol, popsize, dict(vectorized=True, updating="deferred", **_seed_keyword(sd)))
        plan = _engine_for(image_value_stack).DEPlanU16(image_value_stack, image_std_stack, _host(exposure_values), mean_ICRF_array, PCA_array,
                                                        lo, hi, population, data_limits[0], data_limits[1], sd, 2 * int(max_iterations),
                                                        (0.0, 1.95), 0.4, tol, energy_limit, bit_depth, variant)
        st = plan.run(check_every, graph)
        u = plan.population[st["best_index"]].cpu().numpy()
        results.append((_inverse_camera_response_function(mean_ICRF_array, PCA_array, lo + u * (hi - lo), True), st["best_energy"],
                        st["generation"] // 2))
    return _best_restart(results)


def calibration_u16(mean_ICRFs: Sequence, PCA_arrays: Sequence, channel_image_value_stacks, channel_image_std_stacks, exposure_values,
                    lower_PCA_limit: float, upper_PCA_limit: float, bit_depth: int, data_limits=None, energy_limit: float = 0.0,
                    rng_seed: int = 7, max_iterations: int = 1000, popsize: int = 15, restarts: int = 1, variant: int = 0,
                    batched: bool = False):
    """calibration(..., bit_depth=b) with the device solver: torch.uint16 channel stacks of a b-bit camera (initialize_channel_image_stacks(
    ..., bit_depth=b)), every channel solved by solve_channel_u16 (seed rng_seed + c), one after another. The mean ICRFs are required: the
    power-law base needs calibration(..., bit_depth=b) on SciPy's solver.
    batched=True solves all C x `restarts` problems as one engine.DEBatchPlanU16 - channel c's restart r seeded restart_seed(rng_seed + c, r),
    the best restart kept per channel; more than 64 problems go in consecutive batches of at most 64. It needs channel stacks of one shape
    and the same number of PCA components for every channel (ValueError otherwise, never a sequential fallback); the result is array-equal
    to the sequential one.
    -> (ICRF (2**b, C): what engine.merge(..., bit_depth=b) takes, final energies (C,))."""
    bit_depth = engine._check_bit_depth(bit_depth)
    C = len(channel_image_value_stacks)
    if mean_ICRFs is None or len(mean_ICRFs) != C or any(m is None for m in mean_ICRFs):
        raise ValueError("calibration_u16 needs the mean ICRF of every channel: the device solver forms candidates from a mean ICRF only")
    results, energies = [], np.zeros(C)
    if batched:
        restarts = int(restarts)
        if restarts < 1:
            raise ValueError(f"restarts must be >= 1, got {restarts}")
        n_params =[np.shape(b)[1] for b in PCA_arrays]
        if len(set(n_params)) != 1:                                              # (before the batches are cut: one of them might hold one channel only)
            raise ValueError(f"a batched solve needs the same number of PCA components for every problem, got {n_params}")
        idx = [(c, r) for c in range(C) for r in range(restarts)]
        solved = []
        for first in range(0, len(idx), nat.HM_DE_MAX_PROBLEMS):
            part = idx[first:first + nat.HM_DE_MAX_PROBLEMS]
            solved += _solve_batch([mean_ICRFs[c] for c, _ in part], [PCA_arrays[c] for c, _ in part], list(channel_image_value_stacks),
                                   list(channel_image_std_stacks), [c for c, _ in part], [restart_seed(rng_seed + c, r) for c, r in part],
                                   exposure_values, lower_PCA_limit, upper_PCA_limit, _data_limits_u16(data_limits, bit_depth), energy_limit,
                                   max_iterations, popsize, **_device_defaults(solve_channel_u16), bit_depth=bit_depth, variant=variant)
        for c in range(C):
            icrf_c, energies[c], _ = _best_restart(solved[c * restarts:(c + 1) * restarts])
            results.append(icrf_c)
    else:
        for c in range(C):
            icrf_c, energies[c], _ = solve_channel_u16(mean_ICRFs[c], PCA_arrays[c], channel_image_value_stacks[c], channel_image_std_stacks[c],
                                                       exposure_values, lower_PCA_limit, upper_PCA_limit, bit_depth, data_limits, energy_limit,
                                                       rng_seed + c, max_iterations, popsize, restarts=restarts, variant=variant)
            results.append(icrf_c)
    ICRF = np.stack(results, axis=1)
    ICRF += (1 - ICRF[-1, :])[None, :]                                           # :390
    ICRF[0, :] = 0                                                               # :391
    ICRF[ICRF < 0] = 0                                                           # :395-396
    ICRF[ICRF > 1] = 1
    return ICRF, energies


def calibration(mean_ICRFs: Sequence, PCA_arrays: Sequence, channel_image_value_stacks, channel_image_std_stacks, exposure_values,
                lower_PCA_limit: float, upper_PCA_limit: float, initial_function=None,
                data_limits=(gs.LOWER_LIN_LIM, gs.UPPER_LIN_LIM), energy_limit: float = 0.0, rng_seed: int = 7,
                vectorized: bool = True, max_iterations: int = 1000, popsize: int = 15, solver: str = "scipy", batched: bool = False,
                restarts: int = 1, bit_depth: Optional[int] = None):
    """calibration() (:287-405) from arrays: per-channel mean ICRF (or `initial_function`) and PCA basis, the channel stacks
    of initialize_channel_image_stacks. By default the channels are solved one after another on this process's GPU (the reference
    forks one joblib worker per channel, :383; with one process per GPU, give each rank a channel instead).
    solver="device", batched=True solves them CONCURRENTLY, the reference's joblib.Parallel(n_jobs=NUM_OF_CHS) as one
    engine.DEBatchPlan: all C x `restarts` problems in one set of launches per generation, channel c's restart r seeded
    restart_seed(rng_seed + c, r), the best restart kept per channel. It needs channel stacks of one shape and the same number of PCA
    components for every channel (ValueError otherwise, never a sequential fallback); with restarts=1 the result equals the sequential
    solver="device" one bit for bit. `restarts` > 1 without `batched` runs each channel's restarts as a batch, channel after channel.
    bit_depth=b (9..16, solver="scipy" only; the device solver is calibration_u16): torch.uint16 channel stacks of a b-bit camera (initialize_channel_image_stacks(...,
    bit_depth=b)), mean ICRFs and PCA bases of 2**b rows; the result has 2**b rows and is what engine.merge(..., bit_depth=b) takes.
    `data_limits` are DNs of the stacks' depth and are not rescaled: the defaults are 8-bit DNs and wrong for any other depth.
    -> (ICRF (BITS, C) interpolated - (2**b, C) with bit_depth -, final energies (C,))."""
    if bit_depth is not None:
        _scipy_only(bit_depth, solver, batched, int(restarts))
    C = len(channel_image_value_stacks)
    use_mean_ICRF = initial_function is None
    results, energies = [], np.zeros(C)
    if batched:
        if solver != "device":
            raise ValueError('batched=True needs solver="device": the channels run as one batch on the stacks\' backend')
        if not use_mean_ICRF:
            raise NotImplementedError('solver="device" forms candidates from a mean ICRF only; the power-law base (initial_function) needs '
                                      'solver="scipy"')
        restarts = int(restarts)
        if restarts < 1:
            raise ValueError(f"restarts must be >= 1, got {restarts}")
        idx = [(c, r) for c in range(C) for r in range(restarts)]
        solved = _solve_batch([mean_ICRFs[c] for c, _ in idx], [PCA_arrays[c] for c, _ in idx], list(channel_image_value_stacks),
                              list(channel_image_std_stacks), [c for c, _ in idx], [restart_seed(rng_seed + c, r) for c, r in idx],
                              exposure_values, lower_PCA_limit, upper_PCA_limit, data_limits, energy_limit, max_iterations, popsize,
                              **_device_defaults())
        for c in range(C):
            icrf_c, energies[c], _ = _best_restart(solved[c * restarts:(c + 1) * restarts])
            results.append(icrf_c)
    else:
        for c in range(C):
            base = mean_ICRFs[c] if use_mean_ICRF else initial_function
            icrf_c, energies[c], _ = solve_channel(base, PCA_arrays[c], channel_image_value_stacks[c], channel_image_std_stacks[c],
                                                   exposure_values, lower_PCA_limit, upper_PCA_limit, use_mean_ICRF, data_limits,
                                                   energy_limit, rng_seed + c, max_iterations, vectorized, popsize, c, solver=solver,
                                                   restarts=restarts, bit_depth=bit_depth)
            results.append(icrf_c)
    ICRF = np.stack(results, axis=1)
    ICRF += (1 - ICRF[-1, :])[None, :]                                           # :390
    ICRF[0, :] = 0                                                               # :391
    ICRF[ICRF < 0] = 0                                                           # :395-396
    ICRF[ICRF > 1] = 1
    return interpolate_ICRF(ICRF, bits=None if bit_depth is None else 2 ** bit_depth), energies
