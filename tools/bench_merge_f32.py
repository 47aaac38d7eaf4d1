#!/usr/bin/env python3
"""float32 against float64 outputs of the fused merge, in ONE process on one device.

For each shape four distinct stacks are resident and merged round-robin, as in bench.py (no launch finds the previous launch's inputs in
the Infinity Cache). The float64 plan, the float32 plan and - where the float32 plan stores four elements per lane - the float32 plan with
pair stores forced (variant 32) of the SAME stacks take turns: repeat r times a timed region of `steps` back-to-back launches of one kind,
HIP events around the region. Reported per kind: the median of the repeats, their spread (max - min), algorithmic bytes and GB/s; and the
time ratio float32 / float64 next to the byte ratio.

    python tools/bench_merge_f32.py                    # config 2, its std form, config 4's tile
    python tools/bench_merge_f32.py --shapes cfg2 --repeats 9

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
    # name: (frames, H, W, with_std)                               bytes per element float64 -> float32
    "cfg2": (7, 4096, 4096, False),      # BASELINE config 2, val only              15 -> 11
    "cfg2std": (7, 4096, 4096, True),    # ... with std                             79 -> 71
    "cfg4tile": (15, 1024, 8192, False), # one row tile of config 4                 23 -> 19
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg2,cfg2std,cfg4tile")
    ap.add_argument("--steps", type=int, default=40, help="launches per timed region")
    ap.add_argument("--repeats", type=int, default=9, help="timed regions per kind (the kinds alternate)")
    ap.add_argument("--stacks", type=int, default=4, help="distinct resident stacks merged round-robin")
    ap.add_argument("--prewarm-s", type=float, default=0.5)
    a = ap.parse_args()

    import torch
    from camera_linearity_amd import engine
    from camera_linearity_amd.synthetic import synthetic_icrf, synthetic_stack_device
    dev = torch.device("cuda", 0)
    icrf, diff = synthetic_icrf()

    for name in a.shapes.split(","):
        n, H, W, with_std = SHAPES[name]
        kinds = {"f64": [], "f32": []}
        for k in range(a.stacks):
            frames, stds, t = synthetic_stack_device(7 + 100 * k, n, H, W, device=dev, with_std=with_std)
            args = (frames, t, icrf, diff if with_std else None, stds)
            kinds["f64"].append(engine.plan_merge(*args))
            kinds["f32"].append(engine.plan_merge(*args, out_dtype=torch.float32))
            if "out=f32x4" in kinds["f32"][-1].kernels:          # the store-shape A/B: the same kernel with 8-byte stores
                kinds.setdefault("f32_pairs", []).append(engine.plan_merge(*args, out_dtype=torch.float32, variant=32))
        counters = {kind: 0 for kind in kinds}

        def region(kind, steps):
            plans = kinds[kind]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                plans[counters[kind] % len(plans)].launch()
                counters[kind] += 1
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / steps                # us per launch

        t_end = time.perf_counter() + a.prewarm_s                   # clock pre-warm, untimed (as bench.py)
        while time.perf_counter() < t_end:
            for kind in kinds:
                region(kind, 10)
        times = {kind: [] for kind in kinds}
        for _ in range(a.repeats):
            for kind in kinds:                                      # alternating: a drift of the box hits every kind alike
                times[kind].append(region(kind, a.steps))
        line = {"shape": name, "frames": n, "height": H, "width": W, "with_std": with_std, "steps": a.steps, "repeats": a.repeats,
                "resident_stacks": a.stacks, "device": torch.cuda.get_device_name(0)}
        for kind, plans in kinds.items():
            med = statistics.median(times[kind])
            line[kind] = {"kernels": plans[0].kernels, "us": round(med, 2), "spread_us": round(max(times[kind]) - min(times[kind]), 2),
                          "min_us": round(min(times[kind]), 2), "algorithmic_bytes": plans[0].algorithmic_bytes,
                          "GBps": round(plans[0].algorithmic_bytes / med / 1e3, 1)}
        line["time_ratio_f32_over_f64"] = round(line["f32"]["us"] / line["f64"]["us"], 4)
        line["byte_ratio_f32_over_f64"] = round(line["f32"]["algorithmic_bytes"] / line["f64"]["algorithmic_bytes"], 4)
        line["f32_faster_by_us"] = round(line["f64"]["us"] - line["f32"]["us"], 2)
        line["f32_faster_by_more_than_f64_spread"] = bool(line["f64"]["us"] - line["f32"]["us"] > line["f64"]["spread_us"])
        if "f32_pairs" in line:
            line["time_ratio_pairs_over_f64"] = round(line["f32_pairs"]["us"] / line["f64"]["us"], 4)
        print(json.dumps(line), flush=True)
        del kinds, plans
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
