#!/usr/bin/env python3
"""The uint16 merge with its stds from the per-DN STD table (hm_merge_u16_std_table) against the route that materialises them, per bit
depth, in ONE process on one device. The method is tools/bench_merge_std_table.py's.

Per depth, `--stacks` distinct stacks are resident and merged round-robin (no launch finds the previous launch's inputs in the Infinity
Cache). The kinds take turns - repeat r times a timed region of `steps` back-to-back launches of one kind, HIP events around the region:

    table          engine.plan_merge_u16_std_table(...)                                    (hm_merge_u16_std_table)
    materialised   N hm_linearize_u16 launches that write the float64 std frames, then the std-stream merge (hm_merge_u16): the route
                   the entry replaces
    stream         the std-stream merge alone (std frames already resident)
    value          the value-only merge

The routes are compared as bit patterns before anything is timed. Reported per kind: median, spread (max - min), algorithmic bytes, GB/s;
the device bytes each route holds for one stack; and - at `--pipeline-depth`, unless --pipeline-stacks 0 - MergePipeline stacks per second
with std_table against with_std staging (host-resident stacks over PCIe).

    python tools/bench_merge_u16_std_table.py                  # 7 x 4096 x 4096 x 3 at 10, 11, 12, 13 and 16 bits
    python tools/bench_merge_u16_std_table.py --depths 12 --repeats 9

One JSON line per depth, one for the pipeline."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="10,11,12,13,16")
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20, help="launches per timed region")
    ap.add_argument("--repeats", type=int, default=7, help="timed regions per kind (the kinds alternate)")
    ap.add_argument("--stacks", type=int, default=4, help="distinct resident stacks merged round-robin")
    ap.add_argument("--prewarm-s", type=float, default=0.5)
    ap.add_argument("--pipeline-stacks", type=int, default=6, help="stacks streamed through MergePipeline per kind (0: skip)")
    ap.add_argument("--pipeline-depth", type=int, default=12, help="bit depth of the MergePipeline comparison")
    a = ap.parse_args()

    import numpy as np
    import torch
    from camera_linearity_amd import _native as nat
    from camera_linearity_amd import engine
    from camera_linearity_amd.pipeline import MergePipeline
    from camera_linearity_amd.synthetic import synthetic_exposures, synthetic_icrf
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    n, H, W, C_ = a.frames, a.height, a.width, 3
    t = synthetic_exposures(n)
    F64 = torch.float64
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(11)

    def stack_u16(seed, b):
        """tools/bench_merge_u16.py's stacks: DN = clip(round(rad t k), 0, M), k = M / (4 t_mid)."""
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        M = 2 ** b - 1
        rad = torch.rand((H, W, C_), generator=gen, device=dev, dtype=F64) * 4
        k = M / (4 * t[n // 2])
        out = []
        for ti in t:
            x = torch.clamp(torch.round(rad * float(ti * k)), 0, M).to(torch.int32)
            out.append(torch.where(x >= 32768, x - 65536, x).to(torch.int16).view(torch.uint16))
        return out

    for b in [int(x) for x in a.depths.split(",")]:
        icrf, diff = synthetic_icrf(bits=2 ** b)
        table = torch.as_tensor(rng.random((2 ** b, C_)) * 0.01, device=dev)
        kinds = {"table": [], "materialised": [], "stream": [], "value": []}
        held, info = {}, {}
        for k in range(a.stacks):
            frames = stack_u16(7 + 100 * k, b)
            stds = [engine.linearize(f, None, table, bit_depth=b)[0] for f in frames]
            p_tab = engine.plan_merge_u16_std_table(frames, t, icrf, diff, table, bit_depth=b)
            p_str = engine.plan_merge(frames, t, icrf, diff, stds, bit_depth=b)
            p_val = engine.plan_merge(frames, t, icrf, bit_depth=b)

            def materialise(frames=frames, stds=stds, p_str=p_str):
                for f, s in zip(frames, stds):                      # the std frames, written by the linearize kernel into resident buffers
                    rc = nat.lib.hm_linearize_u16(f.data_ptr(), None, table.data_ptr(), None, s.data_ptr(), None, None, f.numel(), C_, C_, b, stream)
                    assert rc == 0
                p_str.launch()
            if k == 0:                                              # the routes agree bit for bit before anything is timed
                p_tab.launch()
                p_val.launch()
                materialise()
                torch.cuda.synchronize()
                for q in ("val", "std"):
                    assert torch.equal(p_tab.outputs[q].view(torch.int64), p_str.outputs[q].view(torch.int64)), (b, q)
                assert torch.equal(p_tab.outputs["val"].view(torch.int64), p_val.outputs["val"].view(torch.int64)), b
                nb = lambda ts: sum(x.numel() * x.element_size() for x in ts)   # noqa: E731
                out_b = nb(p_tab.outputs.values())
                held = {"table": nb(frames) + out_b + table.numel() * 8, "materialised": nb(frames) + nb(stds) + out_b}
                info = {"table": (p_tab.kernels, p_tab.algorithmic_bytes),
                        "materialised": (f"{n} x hm_linearize_u16 + " + p_str.kernels, p_str.algorithmic_bytes + n * 10 * frames[0].numel()),
                        "stream": (p_str.kernels, p_str.algorithmic_bytes), "value": (p_val.kernels, p_val.algorithmic_bytes)}
            kinds["table"].append(p_tab.launch)
            kinds["materialised"].append(materialise)
            kinds["stream"].append(p_str.launch)
            kinds["value"].append(p_val.launch)
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
        line = {"bit_depth": b, "frames": n, "height": H, "width": W, "channels": C_, "steps": a.steps, "repeats": a.repeats,
                "resident_stacks": a.stacks, "device": torch.cuda.get_device_name(0), "device_bytes_held_per_stack": held}
        for kind in kinds:
            med = statistics.median(times[kind])
            line[kind] = {"kernels": info[kind][0], "us": round(med, 2), "spread_us": round(max(times[kind]) - min(times[kind]), 2),
                          "min_us": round(min(times[kind]), 2), "algorithmic_bytes": info[kind][1], "GBps": round(info[kind][1] / med / 1e3, 1)}
        line["table_over_materialised"] = round(line["table"]["us"] / line["materialised"]["us"], 4)
        line["table_over_stream"] = round(line["table"]["us"] / line["stream"]["us"], 4)
        line["table_faster_than_materialised_beyond_spreads"] = bool(
            line["materialised"]["us"] - line["table"]["us"] > line["materialised"]["spread_us"] + line["table"]["spread_us"])
        print(json.dumps(line), flush=True)
        del kinds, p_tab, p_str, p_val, frames, stds, materialise
        torch.cuda.empty_cache()

    if a.pipeline_stacks > 0:                                       # host-resident stacks through the three-stream pipeline
        b = a.pipeline_depth
        icrf, diff = synthetic_icrf(bits=2 ** b)
        table = rng.random((2 ** b, C_)) * 0.01
        host = [rng.integers(0, 2 ** b, size=(H, W, C_), dtype=np.uint16) for _ in range(n)]
        host_std = [np.full((H, W, C_), 0.004) for _ in range(n)]
        rate = {}
        for kind in ("std_table", "with_std"):
            pipe = (MergePipeline(n, H, W, t, icrf, diff, bit_depth=b, std_table=table) if kind == "std_table"
                    else MergePipeline(n, H, W, t, icrf, diff, bit_depth=b, with_std=True))
            total = a.pipeline_stacks + 2

            def fill(k, fv, sv, total=total):
                if k >= total:
                    return False
                if k < pipe.depth:                                  # every slot's staging is filled once; later stacks reuse the bytes
                    for d, s in zip(fv, host):
                        np.copyto(d, s)
                    if sv is not None:
                        for d, s in zip(sv, host_std):
                            np.copyto(d, s)
                return True
            t0 = None
            for k, _, _ in pipe.run(fill):
                if k == 1:                                          # the first two stacks fill the pipeline: untimed
                    t0 = time.perf_counter()
            rate[kind] = round(a.pipeline_stacks / (time.perf_counter() - t0), 2)
            del pipe
            torch.cuda.empty_cache()
        print(json.dumps({"pipeline_bit_depth": b, "frames": n, "height": H, "width": W, "pipeline_stacks_per_s": rate}), flush=True)


if __name__ == "__main__":
    main()
