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
Options: --generations G (default 400), --repeats R (default 5), --check-every K (default 8), --sizes 28,256.

--problems K[,K...] measures the batched plan instead: for every stack size and every K, ONE child process times an engine.DEBatchPlan of
K problems (3 channel stacks, problem k on stack k mod 3 with seed 7 + k: 12 = 3 channels x 4 restarts) next to K sequential engine.DEPlan
solves of the same problems - HIP events around the graph replays of --generations generations, median of --repeats, never stopping
(tol = 0, no generation limit). One JSON line per (stack, K):
  batch_us_per_generation       one batched generation of all K problems
  sequential_us_per_generation  one generation of each of the K single plans, one plan after another (for K = 1: the single plan)
  sequential_over_batch         their ratio; `margin` is the larger of 4 % and the min-max spread of the sequential repetitions, and
  batch_within_margin           batch <= sequential (1 + margin)
Both sides replay their plans' recorded graphs back to back and neither reads a status block in between (the figures come from the
plans' own recording, engine.DEPlan._record / DEBatchPlan._record): the ratio is a device-only figure, not the wall time of
solve_channel or calibration that a caller sees, which adds population set-up, capture and one status read per replay."""
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


def problem(side, N=7, P=5, seed=21):
    import numpy as np
    from camera_linearity_amd import icrf_calibration as ic
    rng = np.random.default_rng(seed)
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


def batch_step(sizes, counts, generations, repeats, check_every):
    import numpy as np
    import torch
    from scipy.stats import qmc
    from camera_linearity_amd import engine
    replays = max(1, generations // check_every)
    gens = replays * check_every

    def timed(graphs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for _ in range(repeats + 1):                              # the first repetition warms up and is dropped
            e0.record()
            for g in graphs:                                      # one plan after another, as K sequential solves run
                for _ in range(replays):
                    g.replay()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / gens)
        return out[1:]
    for side in sizes:
        channels = [problem(side, seed=21 + c) for c in range(3)]
        mean_icrf, pca, _, t = channels[0]
        stacks = [c[2] for c in channels]
        for K in counts:
            pops = np.stack([qmc.Sobol(5, seed=7 + k).random(128) for k in range(K)])
            stack_of = [k % 3 for k in range(K)]
            seeds = [7 + k for k in range(K)]
            batch = engine.DEBatchPlan(stacks, None, t, [mean_icrf] * K, [pca] * K, -1.0, 1.0, pops, 5, 250, seeds, 1 << 40, tol=0.0,
                                       stack_of=stack_of)
            singles = [engine.DEPlan(stacks[stack_of[k]], None, t, mean_icrf, pca, -1.0, 1.0, pops[k], 5, 250, seeds[k], 1 << 40, tol=0.0)
                       for k in range(K)]
            for pl in [batch] + singles:
                pl._record(check_every)
            seq = timed([pl._graph for pl in singles])
            bat = timed([batch._graph])
            for k in range(K):                                    # the same generations ran on both sides: the states must be the same bits
                assert torch.equal(batch.population[k], singles[k].population) and torch.equal(batch.status[k], singles[k].status), k
            b, q = statistics.median(bat), statistics.median(seq)
            margin = max(0.04, (max(seq) - min(seq)) / q)
            print(json.dumps({"step": "batch", "stack": [side, side, 7], "problems": K, "population": 128, "params": 5,
                              "generations": gens, "check_every": check_every, "repeats": repeats,
                              "batch_us_per_generation": round(b, 2), "batch_us_spread": [round(min(bat), 2), round(max(bat), 2)],
                              "sequential_us_per_generation": round(q, 2), "sequential_us_spread": [round(min(seq), 2), round(max(seq), 2)],
                              "sequential_over_batch": round(q / b, 3), "margin": round(margin, 4),
                              "batch_within_margin": bool(b <= q * (1 + margin)), "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    generations, repeats, check_every = opt("--generations", 400), opt("--repeats", 5), opt("--check-every", 8)
    sizes = [int(s) for s in opt("--sizes", "28,256").split(",")]
    if "--step" in sys.argv:
        sys.path.insert(0, str(ROOT))
        if opt("--step", "") == "batch":
            batch_step(sizes, [int(k) for k in opt("--problems", "1").split(",")], generations, repeats, check_every)
        else:
            step(opt("--step", ""), sizes[0], generations, repeats, check_every)
        return
    if "--problems" in sys.argv:                                  # one child for all sizes and problem counts, under its own time limit
        cmd = ["timeout", "-k", "10", "600", sys.executable, str(pathlib.Path(__file__).resolve()), "--step", "batch", "--problems",
               opt("--problems", "1"), "--sizes", ",".join(map(str, sizes)), "--generations", str(generations), "--repeats", str(repeats),
               "--check-every", str(check_every)]
        p = subprocess.run(cmd)
        if p.returncode != 0:
            print(json.dumps({"tool": "bench_de", "failed_step": "batch", "exit_status": p.returncode}))
        sys.exit(p.returncode)
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
