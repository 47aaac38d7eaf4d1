#!/usr/bin/env python3
"""The merge with its stds from the per-DN STD table against the route that materialises them, in ONE process on one device
(DESIGN.md 4.1.2).

Per shape, `--stacks` distinct stacks are resident and merged round-robin (no launch finds the previous launch's inputs in the Infinity
Cache). The kinds take turns - repeat r times a timed region of `steps` back-to-back launches of one kind, HIP events around the region:

    table          engine.plan_merge(std_table=...)                                        (hm_merge_std_table)
    table_loop     the same with the run-time-N kernel forced (variant 10): the A/B of the templated instantiation
    materialised   N hm_linearize_u8 launches that write the std frames, then the std-stream merge: the route to the same output without
                   the table entry point
    stream         the std-stream merge alone (std frames already resident)

Reported per kind: median, spread (max - min), algorithmic bytes, GB/s; the device bytes each route holds for one stack; and - unless
--pipeline-stacks 0 - MergePipeline stacks per second with std_table against with_std staging (host-resident stacks over PCIe).

    python tools/bench_merge_std_table.py                  # 7 x 4096 x 4096 x 3 and config 4's tile
    python tools/bench_merge_std_table.py --shapes cfg3 --repeats 9

One JSON line per shape."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SHAPES = {
    # name: (frames, H, W)                    algorithmic bytes per element: table / std streams
    "cfg3": (7, 4096, 4096),                # config 3's shape without its flat field      23 / 79
    "cfg4tile": (15, 1024, 8192),           # one row tile of config 4                     31 / 151
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3,cfg4tile")
    ap.add_argument("--steps", type=int, default=20, help="launches per timed region")
    ap.add_argument("--repeats", type=int, default=7, help="timed regions per kind (the kinds alternate)")
    ap.add_argument("--stacks", type=int, default=4, help="distinct resident stacks merged round-robin")
    ap.add_argument("--prewarm-s", type=float, default=0.5)
    ap.add_argument("--pipeline-stacks", type=int, default=6, help="stacks streamed through MergePipeline per kind (0: skip)")
    a = ap.parse_args()

    import numpy as np
    import torch
    from camera_linearity_amd import _native as nat
    from camera_linearity_amd import engine
    from camera_linearity_amd.pipeline import MergePipeline
    from camera_linearity_amd.synthetic import synthetic_icrf, synthetic_stack_device
    dev = torch.device("cuda", 0)
    icrf, diff = synthetic_icrf()
    rng = np.random.default_rng(11)
    table = torch.as_tensor(rng.random((256, 3)) * 0.01, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    for name in a.shapes.split(","):
        n, H, W = SHAPES[name]
        kinds = {"table": [], "table_loop": [], "materialised": [], "stream": []}
        held = {}
        for k in range(a.stacks):
            frames, _, t = synthetic_stack_device(7 + 100 * k, n, H, W, device=dev, with_std=False)
            stds = [engine.linearize(f, None, table)[0] for f in frames]
            p_tab = engine.plan_merge(frames, t, icrf, diff, std_table=table)
            p_loop = engine.plan_merge(frames, t, icrf, diff, std_table=table, variant=10)
            p_str = engine.plan_merge(frames, t, icrf, diff, stds)
            if k == 0:                                              # the routes agree bit for bit before anything is timed
                for p in (p_tab, p_loop, p_str):
                    p.launch()
                torch.cuda.synchronize()
                for q in ("val", "std"):
                    assert torch.equal(p_tab.outputs[q].view(torch.int64), p_str.outputs[q].view(torch.int64)), q
                    assert torch.equal(p_loop.outputs[q].view(torch.int64), p_str.outputs[q].view(torch.int64)), q
                nb = lambda ts: sum(x.numel() * x.element_size() for x in ts)   # noqa: E731
                out_b = nb(p_tab.outputs.values())
                held = {"table": nb(frames) + out_b + table.numel() * 8, "materialised": nb(frames) + nb(stds) + out_b}

            def materialise(frames=frames, stds=stds, p_str=p_str):
                for f, s in zip(frames, stds):                      # the std frames, written by the linearize kernel into resident buffers
                    rc = nat.lib.hm_linearize_u8(f.data_ptr(), None, table.data_ptr(), None, s.data_ptr(), None, f.numel(), 3, 3, stream)
                    assert rc == 0
                p_str.launch()
            kinds["table"].append(p_tab.launch)
            kinds["table_loop"].append(p_loop.launch)
            kinds["materialised"].append(materialise)
            kinds["stream"].append(p_str.launch)
            if k == 0:
                info = {"table": (p_tab.kernels, p_tab.algorithmic_bytes), "table_loop": (p_loop.kernels, p_loop.algorithmic_bytes),
                        "materialised": (f"{n} x hm_linearize_u8 + " + p_str.kernels, p_str.algorithmic_bytes + n * 9 * frames[0].numel()),
                        "stream": (p_str.kernels, p_str.algorithmic_bytes)}
        counters = {kind: 0 for kind in kinds}

        def region(kind, steps):
            calls = kinds[kind]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                calls[counters[kind] % len(calls)]()
                counters[kind] += 1
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / steps                # us per launch

        t_end = time.perf_counter() + a.prewarm_s                   # clock pre-warm, untimed (as bench.py)
        while time.perf_counter() < t_end:
            for kind in kinds:
                region(kind, 5)
        times = {kind: [] for kind in kinds}
        for _ in range(a.repeats):
            for kind in kinds:                                      # alternating: a drift of the box hits every kind alike
                times[kind].append(region(kind, a.steps))
        line = {"shape": name, "frames": n, "height": H, "width": W, "steps": a.steps, "repeats": a.repeats, "resident_stacks": a.stacks,
                "device": torch.cuda.get_device_name(0), "device_bytes_held_per_stack": held}
        for kind in kinds:
            med = statistics.median(times[kind])
            line[kind] = {"kernels": info[kind][0], "us": round(med, 2), "spread_us": round(max(times[kind]) - min(times[kind]), 2),
                          "min_us": round(min(times[kind]), 2), "algorithmic_bytes": info[kind][1], "GBps": round(info[kind][1] / med / 1e3, 1)}
        line["table_over_materialised"] = round(line["table"]["us"] / line["materialised"]["us"], 4)
        line["table_over_stream"] = round(line["table"]["us"] / line["stream"]["us"], 4)
        del kinds, p_tab, p_loop, p_str, frames, stds, materialise
        torch.cuda.empty_cache()

        if a.pipeline_stacks > 0:                                   # host-resident stacks through the three-stream pipeline
            host = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(n)]
            host_std = [np.full((H, W, 3), 0.004) for _ in range(n)]
            rate = {}
            for kind in ("std_table", "with_std"):
                pipe = (MergePipeline(n, H, W, t, icrf, diff, std_table=table) if kind == "std_table"
                        else MergePipeline(n, H, W, t, icrf, diff, with_std=True))
                total = a.pipeline_stacks + 2

                def fill(k, fv, sv, total=total):
                    if k >= total:
                        return False
                    if k < pipe.depth:                              # every slot's staging is filled once; later stacks reuse the bytes
                        for d, s in zip(fv, host):
                            np.copyto(d, s)
                        if sv is not None:
                            for d, s in zip(sv, host_std):
                                np.copyto(d, s)
                    return True
                t0 = None
                for k, _, _ in pipe.run(fill):
                    if k == 1:                                      # the first two stacks fill the pipeline: untimed
                        t0 = time.perf_counter()
                rate[kind] = round(a.pipeline_stacks / (time.perf_counter() - t0), 2)
                del pipe
                torch.cuda.empty_cache()
            line["pipeline_stacks_per_s"] = rate
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
