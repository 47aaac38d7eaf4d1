#!/usr/bin/env python3
"""The fused merge on uint16 DN frames (hm_merge_u16) per bit depth, table placement and std mode, next to the uint8 merge of the same
shape and the device's copy rate, in ONE process on one device.

Per depth, `--stacks` distinct stacks are resident and merged round-robin, as bench.py does (no launch finds the previous launch's inputs
in the Infinity Cache). Kinds: value-only and with float64 stds, each under the default dispatch (variant 0) and every forced variant
that is legal - 1 tables in LDS (where they fit), 3 the largest part of the tables in LDS (where a part fits), 2 tables in global memory,
-1 one element per thread. The kinds take turns: repeat r times a timed region of `steps` back-to-back launches of one kind, HIP events
around the region. Before timing, every forced variant's outputs are compared with the default's as bit patterns.

Reported per kind: the kernels, median us per launch, spread (max - min), algorithmic bytes (hm_merge_u16_algorithmic_bytes) and the
fraction of 8 TB/s; per depth and mode the fastest streaming variant and whether the default dispatch is that variant. Anchors of the same
run: the uint8 hm_merge of the same shape (value-only and with std) and the copy rate of the library's copy probe (bench.py's
roofline.copy_GBps).

    python tools/bench_merge_u16.py                        # 7 x 4096 x 4096 x 3, depths 10, 12, 16
    python tools/bench_merge_u16.py --depths 12 --repeats 9

One JSON line per depth, one for the anchors."""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

PEAK_TBPS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="10,12,16")
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=8, help="launches per timed region")
    ap.add_argument("--repeats", type=int, default=7, help="timed regions per kind (the kinds alternate)")
    ap.add_argument("--stacks", type=int, default=4, help="distinct resident stacks merged round-robin")
    ap.add_argument("--prewarm-s", type=float, default=0.5)
    ap.add_argument("--no-generic", action="store_true", help="leave variant -1 out")
    a = ap.parse_args()

    import torch
    from camera_linearity_amd import _native as nat, engine
    from camera_linearity_amd.synthetic import synthetic_exposures, synthetic_icrf, synthetic_stack_device
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    n, H, W, C_ = a.frames, a.height, a.width, 3
    t = synthetic_exposures(n)
    F64 = torch.float64

    def stack_u16(seed, b):
        """synthetic_stack_device's radiance at depth b: DN = clip(round(rad t k), 0, M), k = M / (4 t_mid)."""
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

    def run_kinds(kinds, info):
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
        for kind in kinds:                                          # every kind's first launches (code objects, the LDS limit): untimed
            region(kind, len(kinds[kind]))
        t_end = time.perf_counter() + a.prewarm_s                   # clock pre-warm, untimed (as bench.py)
        while time.perf_counter() < t_end:
            for kind in kinds:
                region(kind, 2)
        times = {kind: [] for kind in kinds}
        for _ in range(a.repeats):
            for kind in kinds:                                      # alternating: a drift of the box hits every kind alike
                times[kind].append(region(kind, a.steps))
        out = {}
        for kind in kinds:
            med = statistics.median(times[kind])
            out[kind] = {"kernels": info[kind][0], "us": round(med, 2), "spread_us": round(max(times[kind]) - min(times[kind]), 2),
                         "min_us": round(min(times[kind]), 2), "algorithmic_bytes": info[kind][1],
                         "frac_of_8TBps": round(info[kind][1] / med / 1e6 / PEAK_TBPS, 4)}
        return out

    stds = [[torch.rand((H, W, C_), dtype=F64, device=dev).mul_(0.004).add_(0.004) for _ in range(n)] for _ in range(a.stacks)]
    common = {"frames": n, "height": H, "width": W, "channels": C_, "steps": a.steps, "repeats": a.repeats, "resident_stacks": a.stacks,
              "device": torch.cuda.get_device_name(0)}

    for b in [int(x) for x in a.depths.split(",")]:
        icrf, diff = synthetic_icrf(bits=2 ** b)
        stacks = [stack_u16(7 + 100 * k, b) for k in range(a.stacks)]
        kinds, info = {}, {}
        for mode in ("val", "std"):
            std = mode == "std"
            fits = (16 if std else 8) * (1 + C_) * 2 ** b <= 160 * 1024
            part = (std and 8 * (2 + C_) * 2 ** b <= 160 * 1024) or (16 if std else 8) * 2 ** b <= 160 * 1024
            variants = [0, 2] + ([1] if fits else []) + ([3] if part else []) + ([] if a.no_generic else [-1])
            ref = None
            for v in variants:
                plans = [engine.plan_merge(stacks[k], t, icrf, diff if mode == "std" else None, stds[k] if mode == "std" else None,
                                           bit_depth=b, variant=v) for k in range(a.stacks)]
                plans[0].launch()
                torch.cuda.synchronize()
                if ref is None:
                    ref = {q: o.clone() for q, o in plans[0].outputs.items()}
                for q, o in plans[0].outputs.items():               # the variants agree bit for bit
                    assert torch.equal(o.view(torch.int64), ref[q].view(torch.int64)), (b, mode, v, q)
                kind = f"{mode}/v{v}"
                kinds[kind] = [p.launch for p in plans]
                info[kind] = (plans[0].kernels, plans[0].algorithmic_bytes)
            del ref
        line = dict(common, bit_depth=b, kinds=run_kinds(kinds, info))
        for mode in ("val", "std"):
            stream = {k: v["us"] for k, v in line["kinds"].items() if k.startswith(mode) and k[-2:] in ("v1", "v2", "v3")}
            best = min(stream, key=stream.get)
            line[f"{mode}_fastest_stream"] = best
            line[f"{mode}_default_is_fastest"] = line["kinds"][best]["kernels"] == line["kinds"][f"{mode}/v0"]["kernels"]
        print(json.dumps(line), flush=True)
        del kinds, stacks, plans
        torch.cuda.empty_cache()

    # anchors: the uint8 merge of the same shape, and the copy rate
    icrf8, diff8 = synthetic_icrf()
    kinds, info = {"u8_val": [], "u8_std": []}, {}
    for k in range(a.stacks):
        frames, _, t8 = synthetic_stack_device(7 + 100 * k, n, H, W, device=dev)
        pv = engine.plan_merge(frames, t8, icrf8)
        ps = engine.plan_merge(frames, t8, icrf8, diff8, stds[k])
        kinds["u8_val"].append(pv.launch)
        kinds["u8_std"].append(ps.launch)
        info["u8_val"], info["u8_std"] = (pv.kernels, pv.algorithmic_bytes), (ps.kernels, ps.algorithmic_bytes)
    line = dict(common, anchors=run_kinds(kinds, info))
    src, dst = pv.outputs["val"], ps.outputs["val"]
    nbytes = src.numel() * 8
    st = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(20):
        nat.check(nat.lib.hm_debug_copy_probe(src.data_ptr(), dst.data_ptr(), nbytes, st), "copy probe")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(100):
        x, y = (src, dst) if k % 2 == 0 else (dst, src)
        nat.check(nat.lib.hm_debug_copy_probe(x.data_ptr(), y.data_ptr(), nbytes, st), "copy probe")
    e1.record()
    torch.cuda.synchronize()
    line["copy_GBps"] = round(2 * nbytes / (e0.elapsed_time(e1) * 1e-3 / 100) / 1e9, 1)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
