#!/usr/bin/env python3
"""The merge reading float32 std frames as they are against the float64-std merge and against today's route for float32 inputs (widen,
then merge), in ONE process on one device.

Per shape, `--stacks` distinct stacks are resident and merged round-robin, as bench.py does (no launch finds the previous launch's inputs
in the Infinity Cache). The kinds take turns - repeat r times a timed region of `steps` back-to-back launches of one kind, HIP events
around the region:

    f64        (a) the float64-std plan                                                       (hm_merge)
    f32        (b) the float32-std plan                                                       (hm_merge_std_f32)
    widen      (c) the route float32 inputs took before: N .to(float64) launches into resident buffers, then (a)
    f32_out32  (d) (b) with out_dtype=float32

Reported per kind: median us per launch, spread (max - min), algorithmic bytes and achieved TB/s from each plan's algorithmic_bytes (the
widening's 12 N bytes per element added for (c)), and the device bytes each route holds for one stack; and - unless --pipeline-stacks 0 -
MergePipeline(with_std=True) stacks per second with std_dtype float64 against float32 (host-resident stacks over PCIe).

    python tools/bench_merge_std_f32.py                  # 7 x 4096 x 4096 x 3 + std, the same + flat field, and config 4's tile
    python tools/bench_merge_std_f32.py --shapes cfg3std --repeats 9

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
    # name: (frames, H, W, flat field)         algorithmic bytes per element: float32 stds / float64 stds
    "cfg3std": (7, 4096, 4096, False),       # config 3's stack with std                    51 / 79
    "cfg3flat": (7, 4096, 4096, True),       # ... and its flat field (uint8 value, float64 std)   60 / 88
    "cfg4tile": (15, 1024, 8192, False),     # one row tile of config 4 with std            91 / 151
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg3std,cfg3flat,cfg4tile")
    ap.add_argument("--steps", type=int, default=12, help="launches per timed region")
    ap.add_argument("--repeats", type=int, default=7, help="timed regions per kind (the kinds alternate)")
    ap.add_argument("--stacks", type=int, default=4, help="distinct resident stacks merged round-robin")
    ap.add_argument("--prewarm-s", type=float, default=0.5)
    ap.add_argument("--pipeline-stacks", type=int, default=6, help="stacks streamed through MergePipeline per kind (0: skip)")
    a = ap.parse_args()

    import numpy as np
    import torch
    from camera_linearity_amd import engine
    from camera_linearity_amd.pipeline import MergePipeline
    from camera_linearity_amd.synthetic import synthetic_icrf, synthetic_stack_device
    dev = torch.device("cuda", 0)
    icrf, diff = synthetic_icrf()
    rng = np.random.default_rng(13)
    F32, F64 = torch.float32, torch.float64

    for name in a.shapes.split(","):
        n, H, W, with_flat = SHAPES[name]
        kinds = {"f64": [], "f32": [], "widen": [], "f32_out32": []}
        held, info = {}, {}
        fkw = {}
        if with_flat:
            g = torch.Generator(device=dev).manual_seed(5)
            fkw = dict(flat=torch.randint(180, 230, (H, W, 3), dtype=torch.uint8, device=dev, generator=g), ff_mean=[0.8, 0.81, 0.79],
                       flat_std=torch.full((H, W, 3), 0.002, dtype=F64, device=dev), ff_std_mean=[0.002] * 3)
        for k in range(a.stacks):
            frames, stds64, t = synthetic_stack_device(7 + 100 * k, n, H, W, device=dev, with_std=True)
            stds32 = [s.to(F32) for s in stds64]
            for d, s in zip(stds64, stds32):                        # the float64 frames hold the widened float32 values: the routes must agree bit for bit
                d.copy_(s)
            p64 = engine.plan_merge(frames, t, icrf, diff, stds64, **fkw)
            p32 = engine.plan_merge(frames, t, icrf, diff, stds32, **fkw)
            p32o = engine.plan_merge(frames, t, icrf, diff, stds32, out_dtype=F32, **fkw)
            if k == 0:
                for p in (p64, p32, p32o):
                    p.launch()
                torch.cuda.synchronize()
                for q in ("val", "std"):
                    assert torch.equal(p32.outputs[q].view(torch.int64), p64.outputs[q].view(torch.int64)), q
                    assert torch.equal(p32o.outputs[q].view(torch.int32), p64.outputs[q].to(F32).view(torch.int32)), q
                nb = lambda ts: sum(x.numel() * x.element_size() for x in ts)   # noqa: E731
                extra = nb([v for key, v in fkw.items() if key in ("flat", "flat_std")])
                held = {"f64": nb(frames) + nb(stds64) + nb(p64.outputs.values()) + extra,
                        "f32": nb(frames) + nb(stds32) + nb(p32.outputs.values()) + extra,
                        "widen": nb(frames) + nb(stds32) + nb(stds64) + nb(p64.outputs.values()) + extra,
                        "f32_out32": nb(frames) + nb(stds32) + nb(p32o.outputs.values()) + extra}
                info = {"f64": (p64.kernels, p64.algorithmic_bytes), "f32": (p32.kernels, p32.algorithmic_bytes),
                        "widen": (f"{n} x .to(float64) + " + p64.kernels, p64.algorithmic_bytes + n * 12 * frames[0].numel()),
                        "f32_out32": (p32o.kernels, p32o.algorithmic_bytes)}

            def widen(stds32=stds32, stds64=stds64, p64=p64):
                for d, s in zip(stds64, stds32):                    # what s.to(float64) launches, into resident buffers (no allocator in the loop)
                    d.copy_(s)
                p64.launch()
            kinds["f64"].append(p64.launch)
            kinds["f32"].append(p32.launch)
            kinds["widen"].append(widen)
            kinds["f32_out32"].append(p32o.launch)
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
                region(kind, 4)
        times = {kind: [] for kind in kinds}
        for _ in range(a.repeats):
            for kind in kinds:                                      # alternating: a drift of the box hits every kind alike
                times[kind].append(region(kind, a.steps))
        line = {"shape": name, "frames": n, "height": H, "width": W, "flat": with_flat, "steps": a.steps, "repeats": a.repeats,
                "resident_stacks": a.stacks, "device": torch.cuda.get_device_name(0), "device_bytes_held_per_stack": held}
        for kind in kinds:
            med = statistics.median(times[kind])
            line[kind] = {"kernels": info[kind][0], "us": round(med, 2), "spread_us": round(max(times[kind]) - min(times[kind]), 2),
                          "min_us": round(min(times[kind]), 2), "algorithmic_bytes": info[kind][1], "TBps": round(info[kind][1] / med / 1e6, 3)}
        line["f32_over_f64"] = round(line["f32"]["us"] / line["f64"]["us"], 4)
        line["f32_over_widen"] = round(line["f32"]["us"] / line["widen"]["us"], 4)
        assert line["f32"]["us"] < line["widen"]["us"], "the float32-std plan must beat widening + the float64-std plan"
        del kinds, p64, p32, p32o, frames, stds32, stds64, widen, fkw
        torch.cuda.empty_cache()

        if a.pipeline_stacks > 0:                                   # host-resident stacks through the three-stream pipeline
            host = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(n)]
            host_std = [np.full((H, W, 3), 0.004, dtype=np.float32) for _ in range(n)]
            rate = {}
            for kind, sdt in (("std_f64", F64), ("std_f32", F32)):
                pipe = MergePipeline(n, H, W, t, icrf, diff, with_std=True, std_dtype=sdt)
                total = a.pipeline_stacks + 2

                def fill(k, fv, sv, total=total, pipe=pipe):
                    if k >= total:
                        return False
                    if k < pipe.depth:                              # every slot's staging is filled once; later stacks reuse the bytes
                        for d, s in zip(fv, host):
                            np.copyto(d, s)
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
