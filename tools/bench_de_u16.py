#!/usr/bin/env python3
"""Generations per second of the ICRF-calibration differential evolution for 9- to 16-bit cameras: solve_channel_u16 - graph replay and
eager launches - against the SciPy-driven solve_channel(..., bit_depth=b, vectorized=True), by tools/bench_de.py's protocol: the same
synthetic camera at depth b (5 PCA components, SciPy's Sobol population of 128 members), the same seed and the same fixed number of
generations (tol = 0 and energy_limit = 0: neither stops early). Stack sizes 28 x 28 x 7 (a 4096-square image at the reference's
data_spacing of 150) and 256 x 256 x 7, depths 10, 12 and 16.

Without --step this is the driver: every (stack, depth) runs in a child process of its own under `timeout`, one after another, and the
first failure ends the run. A child prints one JSON line per mode (scipy, device-graph, device-eager):
  wall_us_per_generation    wall time of the whole solve call (population set-up, plan, graph capture, solve, result) / generations, median
                            of --repeats calls after one warm-up call. SciPy's calls stop repeating once --scipy-budget seconds are used
                            (at 16 bits a generation builds 128 rows of 65536 entries on the host): `repeats` in the line says how many ran.
  device_us_per_generation  (device modes) HIP events around `check_every` generations of an engine.DEPlanU16, replayed or launched / check_every
After them, with --trace DIR, one `rocprofv3 --kernel-trace --stats` run of its own per depth (28 x 28 x 7, 40 eager generations) gives
k_de_trial_u16's average duration next to the energy and select kernels' (one JSON line per depth; "not measured" if the profiler is
missing or fails - the timings above do not depend on it). The driver ends with a summary line of the ratios.
--step solve --modes device-graph[,...] --sizes N --depths B runs one child's work for those modes alone (how two builds of the library
were compared: HDRMERGE_LIB names the other one).
Options: --generations G (400), --repeats R (5), --check-every K (8), --sizes 28,256, --depths 10,12,16, --scipy-budget S (60), --trace DIR.

--problems K[,K...] measures the batched plan instead, by tools/bench_de.py --problems' protocol: for every (stack, depth) ONE child process
times, for every K, an engine.DEBatchPlanU16 of K problems (3 channel stacks, problem k on stack k mod 3 with seed 7 + k) next to K
engine.DEPlanU16 plans of the same problems replayed one after another - HIP events around the graph replays of --generations generations,
the two sides alternating region by region, median of --repeats regions after one dropped warm-up region each, never stopping (tol = 0, no
generation limit). Afterwards every state array and status block of the two sides is compared as bytes. One JSON line per (stack, depth, K):
batch_us_per_generation (one batched generation of all K problems), sequential_us_per_generation (one generation of each of the K single
plans in turn), their spreads over the regions, sequential_over_batch, and batch_within_margin (batch <= sequential (1 + margin), margin
the larger of 4 % and the sequential regions' min-max spread)."""
import csv
import json
import pathlib
import shutil
import statistics
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
MODES = ("scipy", "device-graph", "device-eager")
S, P = 128, 5


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def problem(side, depth, N=7, seed=21):
    import numpy as np
    from camera_linearity_amd import icrf_calibration as ic
    rng = np.random.default_rng(seed)
    n = 2 ** depth
    t = 1e-3 * 2.0 ** np.arange(N)
    xs = np.linspace(0, 1, n)
    pca = np.stack([np.sin(np.pi * (m + 1) * xs) / (m + 1) for m in range(P)], axis=1) * 0.1
    mean_icrf = 0.5 * xs + 0.5 * xs ** 2                          # (xs ** 2 has a first step of 2.3e-10 at 16 bits)
    true_icrf, ok = ic.candidate_icrfs(np.array([0.6, -0.3, 0.2, 0.1, -0.1]), mean_icrf, pca)
    assert ok[0]
    lin = np.clip((rng.random((side, side)) * 2.5 / t[-1])[..., None] * t, 0, 1)
    dn = np.clip(np.around(np.interp(lin, true_icrf[0], xs) * (n - 1)), 0, n - 1).astype(np.uint16)
    stacks, _, tt = ic.initialize_channel_image_stacks([dn[:, :, None, i] for i in range(N)], t, None, 1, bit_depth=depth)
    return mean_icrf, pca, stacks[0], tt, (5 << (depth - 8), 250 << (depth - 8))


def plan_of(side, depth):
    import numpy as np
    from scipy.stats import qmc
    from camera_linearity_amd import engine
    mean_icrf, pca, stack, t, limits = problem(side, depth)
    pop = qmc.Sobol(P, seed=7).random(S)
    return engine.DEPlanU16(stack, None, t, mean_icrf, pca, -1.0, 1.0, np.asarray(pop), limits[0], limits[1], 7, 1 << 40, tol=0.0,
                            bit_depth=depth)


def solve_step(side, depth, generations, repeats, check_every, scipy_budget):
    import torch
    from camera_linearity_amd import icrf_calibration as ic
    mean_icrf, pca, stack, t, limits = problem(side, depth)
    base = dict(data_limits=limits, seed=7, max_iterations=generations // 2, tol=0.0, energy_limit=0.0)
    for mode in opt("--modes", ",".join(MODES)).split(","):
        def solve(**over):
            t0 = time.perf_counter()
            if mode == "scipy":
                icrf, e, n_it = ic.solve_channel(mean_icrf, pca, stack, None, t, -1.0, 1.0, vectorized=True, bit_depth=depth, **dict(base, **over))
            else:
                icrf, e, n_it = ic.solve_channel_u16(mean_icrf, pca, stack, None, t, -1.0, 1.0, depth, check_every=check_every,
                                                     graph=mode == "device-graph", **dict(base, **over))
            torch.cuda.synchronize()
            return time.perf_counter() - t0, e, n_it
        solve(max_iterations=4)                                   # warm-up: code objects, SciPy imports
        runs, started = [], time.perf_counter()
        while len(runs) < repeats and (not runs or mode != "scipy" or time.perf_counter() - started < scipy_budget):
            runs.append(solve())
        assert all(r[2] == generations // 2 for r in runs), [r[2] for r in runs]
        wall = statistics.median(r[0] for r in runs)
        res = {"step": mode, "stack": [side, side, 7], "bit_depth": depth, "generations": generations, "population": S, "params": P,
               "repeats": len(runs), "wall_us_per_generation": round(wall * 1e6 / generations, 2),
               "wall_us_spread": [round(min(r[0] for r in runs) * 1e6 / generations, 2), round(max(r[0] for r in runs) * 1e6 / generations, 2)],
               "generations_per_s": round(generations / wall, 1), "final_energy": runs[0][1], "device": torch.cuda.get_device_name(0)}
        if mode != "scipy":
            plan = plan_of(side, depth)
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


def batch_step(side, depth, counts, generations, repeats, check_every):
    """--problems: an engine.DEBatchPlanU16 of K problems next to K engine.DEPlanU16 plans replayed one after another, in this process,
    the two sides alternating region by region (tools/bench_de.py --problems' protocol at depth `depth`)."""
    import numpy as np
    import torch
    from scipy.stats import qmc
    from camera_linearity_amd import engine
    replays = max(1, generations // check_every)
    gens = replays * check_every

    def region(graphs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for g in graphs:                                          # one plan after another, as K sequential solves run
            for _ in range(replays):
                g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / gens
    channels = [problem(side, depth, seed=21 + c) for c in range(3)]
    mean_icrf, pca, _, t, limits = channels[0]
    stacks = [c[2] for c in channels]
    for K in counts:
        pops = np.stack([qmc.Sobol(P, seed=7 + k).random(S) for k in range(K)])
        stack_of = [k % 3 for k in range(K)]
        seeds = [7 + k for k in range(K)]
        batch = engine.DEBatchPlanU16(stacks, None, t, [mean_icrf] * K, [pca] * K, -1.0, 1.0, pops, limits[0], limits[1], seeds, 1 << 40, tol=0.0,
                                      stack_of=stack_of, bit_depth=depth)
        singles = [engine.DEPlanU16(stacks[stack_of[k]], None, t, mean_icrf, pca, -1.0, 1.0, pops[k], limits[0], limits[1], seeds[k], 1 << 40,
                                    tol=0.0, bit_depth=depth) for k in range(K)]
        for pl in [batch] + singles:
            pl._record(check_every)
        seq, bat = [], []
        for _ in range(repeats + 1):                              # alternating; the first region of either side warms up and is dropped
            seq.append(region([pl._graph for pl in singles]))
            bat.append(region([batch._graph]))
        seq, bat = seq[1:], bat[1:]
        torch.cuda.synchronize()
        # the same generations ran on both sides: the states must be the same bytes (reported in the line, and the run ends if they are not)
        differ = [(k, name) for k in range(K) for name in ("population", "energies", "trial", "trial_energies", "icrf", "valid", "status")
                  if not torch.equal(getattr(batch, name)[k].view(torch.uint8), getattr(singles[k], name).view(torch.uint8))]
        b, q = statistics.median(bat), statistics.median(seq)
        margin = max(0.04, (max(seq) - min(seq)) / q)
        print(json.dumps({"step": "batch", "stack": [side, side, 7], "bit_depth": depth, "problems": K, "population": S, "params": P,
                          "generations": gens, "check_every": check_every, "repeats": repeats,
                          "batch_us_per_generation": round(b, 2), "batch_us_spread": [round(min(bat), 2), round(max(bat), 2)],
                          "sequential_us_per_generation": round(q, 2), "sequential_us_spread": [round(min(seq), 2), round(max(seq), 2)],
                          "sequential_over_batch": round(q / b, 3), "margin": round(margin, 4),
                          "batch_within_margin": bool(b <= q * (1 + margin)), "states_equal": not differ,
                          "device": torch.cuda.get_device_name(0)}), flush=True)
        if differ:
            sys.exit(f"batch and single plans differ: {differ}")
        del batch, singles
        torch.cuda.empty_cache()


def kernels_step(side, depth, generations):
    """the launches a kernel trace is taken of: `generations` eager generations of one plan"""
    import torch
    plan = plan_of(side, depth)
    for _ in range(generations + 1):
        plan.launch()
    torch.cuda.synchronize()
    assert plan.read_status()["generation"] == generations


def trace(depth, out_dir):
    """-> one JSON-able dict: average kernel durations of a generation at `depth`, from a rocprofv3 run of its own"""
    res = {"step": "kernel-trace", "stack": [28, 28, 7], "bit_depth": depth, "population": S, "params": P}
    if shutil.which("rocprofv3") is None:
        return dict(res, kernels="not measured: no rocprofv3")
    d = pathlib.Path(out_dir) / f"trace_b{depth}"
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(d), "--",
           sys.executable, str(pathlib.Path(__file__).resolve()), "--step", "kernels", "--sizes", "28", "--depths", str(depth), "--generations", "40"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    files = sorted(d.glob("**/*kernel_stats.csv"))
    if p.returncode != 0 or not files:
        return dict(res, kernels=f"not measured: rocprofv3 exit status {p.returncode}", exit_status=p.returncode)
    rows = list(csv.DictReader(files[0].open()))
    res["kernels"] = {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2)}
                      for r in rows if any(k in r["Name"] for k in ("k_de_", "k_energy_"))}
    return res


def main():
    generations, repeats, check_every = opt("--generations", 400), opt("--repeats", 5), opt("--check-every", 8)
    sizes = [int(s) for s in opt("--sizes", "28,256").split(",")]
    depths = [int(b) for b in opt("--depths", "10,12,16").split(",")]
    budget = opt("--scipy-budget", 60.0)
    if "--step" in sys.argv:
        sys.path.insert(0, str(ROOT))
        if opt("--step", "") == "kernels":
            kernels_step(sizes[0], depths[0], generations)
        elif opt("--step", "") == "batch":
            batch_step(sizes[0], depths[0], [int(k) for k in opt("--problems", "1").split(",")], generations, repeats, check_every)
        else:
            solve_step(sizes[0], depths[0], generations, repeats, check_every, budget)
        return
    if "--problems" in sys.argv:                                  # one child per (stack, depth) for all problem counts, under its own time limit
        for side in sizes:
            for depth in depths:
                cmd = ["timeout", "-k", "10", "300", sys.executable, str(pathlib.Path(__file__).resolve()), "--step", "batch", "--problems",
                       opt("--problems", "1"), "--sizes", str(side), "--depths", str(depth), "--generations", str(generations),
                       "--repeats", str(repeats), "--check-every", str(check_every)]
                p = subprocess.run(cmd)
                if p.returncode != 0:                             # stop at the first failure: start nothing more on the GPU
                    print(json.dumps({"tool": "bench_de_u16", "failed_step": "batch", "stack_side": side, "bit_depth": depth,
                                      "exit_status": p.returncode}))
                    sys.exit(p.returncode)
        return
    results = []
    for side in sizes:
        for depth in depths:                                      # one child per (stack, depth) under its own time limit; stop at the first failure
            cmd = ["timeout", "-k", "10", str(int(240 + 8 * budget)), sys.executable, str(pathlib.Path(__file__).resolve()), "--step", "solve",
                   "--sizes", str(side), "--depths", str(depth), "--generations", str(generations), "--repeats", str(repeats),
                   "--check-every", str(check_every), "--scipy-budget", str(budget)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode != 0:
                print(json.dumps({"tool": "bench_de_u16", "failed_step": "solve", "stack_side": side, "bit_depth": depth, "exit_status": p.returncode}))
                sys.exit(p.returncode)
            results += [json.loads(line) for line in p.stdout.strip().splitlines() if line.startswith("{")]
    if "--trace" in sys.argv:
        for depth in depths:
            r = trace(depth, opt("--trace", ""))
            print(json.dumps(r), flush=True)
            if r.get("exit_status") in (124, 134, 137, 139):      # a hang or a fault: start nothing more on the GPU
                sys.exit(r["exit_status"])
    summary = {"tool": "bench_de_u16", "cases": []}
    for side in sizes:
        for depth in depths:
            r = {x["step"]: x for x in results if x["stack"][0] == side and x["bit_depth"] == depth}
            w = {m: r[m]["wall_us_per_generation"] for m in MODES}
            summary["cases"].append({"stack": [side, side, 7], "bit_depth": depth, "scipy_over_device_graph": round(w["scipy"] / w["device-graph"], 2),
                                     "scipy_over_device_eager": round(w["scipy"] / w["device-eager"], 2),
                                     "eager_over_graph": round(w["device-eager"] / w["device-graph"], 2)})
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
