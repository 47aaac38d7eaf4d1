#!/usr/bin/env python3
"""Generations per second of the ICRF-calibration differential evolution: solve_channel(solver="device") - graph replay and eager launches -
against the SciPy-driven solve_channel(vectorized=True), on the same synthetic problem (5 PCA components, SciPy's Sobol population of 128
members), the same seed and the same fixed number of generations (tol = 0 and energy_limit = 0: neither stops early). Stack sizes:
28 x 28 x 7 (a 4096-square image at the reference's data_spacing of 150) and 256 x 256 x 7.

Without --step this is the driver: every GPU step runs in a child process of its own under `timeout`, one after another, and the first
failure ends the run (`&&` semantics). Each step prints one JSON line; the driver prints them and a summary line with the ratios.
  wall_us_per_generation    wall time of the whole solve_channel call (population set-up, plan, graph capture, solve, result) / generations,
                            median of --repeats calls after one warm-up call
  device_us_per_generation  (device steps) HIP events around graph replays of `check_every` generations / check_every
Options: --generations G (default 400), --repeats R (default 5), --check-every K (default 8), --sizes 28,256."""
import json
import pathlib
import statistics
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
STEPS = ("scipy", "device-graph", "device-eager")


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def problem(side, N=7, P=5):
    import numpy as np
    from camera_linearity_amd import icrf_calibration as ic
    rng = np.random.default_rng(21)
    t = 1e-3 * 2.0 ** np.arange(N)
    xs = np.linspace(0, 1, 256)
    pca = np.stack([np.sin(np.pi * (m + 1) * xs) / (m + 1) for m in range(P)], axis=1) * 0.1
    mean_icrf = xs ** 2.0
    true_icrf, ok = ic.candidate_icrfs(np.array([0.6, -0.3, 0.2, 0.1, -0.1][:P]), mean_icrf, pca)
    assert ok[0]
    lin = np.clip((rng.random((side, side)) * 2.5 / t[-1])[..., None] * t, 0, 1)
    dn = np.clip(np.around(np.interp(lin, true_icrf[0], xs) * 255), 0, 255).astype(np.uint8)
    stacks, _, tt = ic.initialize_channel_image_stacks([dn[:, :, None, i] for i in range(N)], t, None, 1)
    return mean_icrf, pca, stacks[0], tt


def step(mode, side, generations, repeats, check_every):
    import torch
    from camera_linearity_amd import engine, icrf_calibration as ic
    mean_icrf, pca, stack, t = problem(side)
    kw = dict(seed=7, max_iterations=generations // 2, tol=0.0, energy_limit=0.0)
    if mode != "scipy":
        kw.update(solver="device", check_every=check_every, graph=mode == "device-graph")

    def solve(**over):
        t0 = time.perf_counter()
        icrf, e, n_it = ic.solve_channel(mean_icrf, pca, stack, None, t, -1.0, 1.0, **dict(kw, **over))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, e, n_it
    solve(max_iterations=4)                                       # warm-up: code objects, SciPy imports
    runs = [solve() for _ in range(repeats)]
    assert all(r[2] == generations // 2 for r in runs), [r[2] for r in runs]
    wall = statistics.median(r[0] for r in runs)
    res = {"step": mode, "stack": [side, side, 7], "generations": generations, "population": 128, "params": 5,
           "wall_us_per_generation": round(wall * 1e6 / generations, 2), "wall_us_spread": [round(min(r[0] for r in runs) * 1e6 / generations, 2),
                                                                                            round(max(r[0] for r in runs) * 1e6 / generations, 2)],
           "generations_per_s": round(generations / wall, 1), "final_energy": runs[0][1], "device": torch.cuda.get_device_name(0)}
    if mode != "scipy":
        import numpy as np
        from scipy.stats import qmc
        pop = qmc.Sobol(5, seed=7).random(128)
        plan = engine.DEPlan(stack, None, t, mean_icrf, pca, -1.0, 1.0, np.asarray(pop), 5, 250, 7, 1 << 40, tol=0.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 50
        if mode == "device-graph":
            plan._record(check_every)
            fn = plan._graph.replay
        else:
            def fn():
                for _ in range(check_every):
                    plan.launch()
        fn()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res["device_us_per_generation"] = round(e0.elapsed_time(e1) * 1e3 / (reps * check_every), 2)
        res["check_every"] = check_every
    print(json.dumps(res), flush=True)


def main():
    generations, repeats, check_every = opt("--generations", 400), opt("--repeats", 5), opt("--check-every", 8)
    sizes = [int(s) for s in opt("--sizes", "28,256").split(",")]
    if "--step" in sys.argv:
        sys.path.insert(0, str(ROOT))
        step(opt("--step", ""), sizes[0], generations, repeats, check_every)
        return
    results = []
    for side in sizes:
        for mode in STEPS:                                        # one child per GPU step, each under its own time limit; stop at the first failure
            cmd = ["timeout", "-k", "10", "240", sys.executable, str(pathlib.Path(__file__).resolve()), "--step", mode, "--sizes", str(side),
                   "--generations", str(generations), "--repeats", str(repeats), "--check-every", str(check_every)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode != 0:
                print(json.dumps({"tool": "bench_de", "failed_step": mode, "stack_side": side, "exit_status": p.returncode}))
                sys.exit(p.returncode)
            results.append(json.loads(p.stdout.strip().splitlines()[-1]))
    summary = {"tool": "bench_de", "cases": []}
    for side in sizes:
        r = {x["step"]: x for x in results if x["stack"][0] == side}
        summary["cases"].append({"stack": [side, side, 7],
                                 "scipy_over_device_graph": round(r["scipy"]["wall_us_per_generation"] / r["device-graph"]["wall_us_per_generation"], 2),
                                 "scipy_over_device_eager": round(r["scipy"]["wall_us_per_generation"] / r["device-eager"]["wall_us_per_generation"], 2),
                                 "eager_over_graph": round(r["device-eager"]["wall_us_per_generation"] / r["device-graph"]["wall_us_per_generation"], 2)})
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
