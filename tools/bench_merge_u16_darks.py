#!/usr/bin/env python3
"""The hot-pixel pass of the uint16 merge (hm_merge_u16_darks: merge_u16_scan_hot + merge_u16_patch_hot) per hot-pixel density, next to
hm_merge_u16 without maps and to the uint8 hm_merge with uint8 maps at the same densities, in ONE process on one device.

tools/bench_merge_u16.py's method: `--stacks` distinct stacks are resident and merged round-robin (no launch finds the previous launch's
inputs in the Infinity Cache), the kinds take turns - repeat r times a timed region of `steps` back-to-back launches of one kind, HIP
events around the region. Every frame has a dark map of its own (7 distinct maps), the same maps for every stack; a share `density` of
each map's elements is hot, independently per map; the recommended workspace. Before timing, the outputs of the density-0 kind are compared
with hm_merge_u16's as bit patterns.

Reported per kind: the kernels, median us per launch, spread (max - min), algorithmic bytes and the fraction of 8 TB/s.

    python tools/bench_merge_u16_darks.py                  # 7 x 4096 x 4096 x 3 at 12 bits, densities 0, 1e-4, 1e-3, 1e-2

One JSON line."""
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
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--densities", default="0,1e-4,1e-3,1e-2")
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--median-k", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8, help="launches per timed region")
    ap.add_argument("--repeats", type=int, default=7, help="timed regions per kind (the kinds alternate)")
    ap.add_argument("--stacks", type=int, default=4, help="distinct resident stacks merged round-robin")
    ap.add_argument("--prewarm-s", type=float, default=0.5)
    a = ap.parse_args()

    import torch
    from camera_linearity_amd import engine
    from camera_linearity_amd.synthetic import synthetic_exposures, synthetic_icrf, synthetic_stack_device
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to time without one"
    dev = torch.device("cuda", 0)
    n, H, W, C_, b, k = a.frames, a.height, a.width, 3, a.depth, a.median_k
    t = synthetic_exposures(n)
    F64 = torch.float64
    densities = [float(x) for x in a.densities.split(",")]

    def stack_u16(seed):
        """tools/bench_merge_u16.py's stack: DN = clip(round(rad t k), 0, M), k = M / (4 t_mid)."""
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        M = 2 ** b - 1
        rad = torch.rand((H, W, C_), generator=gen, device=dev, dtype=F64) * 4
        scale = M / (4 * t[n // 2])
        out = []
        for ti in t:
            x = torch.clamp(torch.round(rad * float(ti * scale)), 0, M).to(torch.int32)
            out.append(torch.where(x >= 32768, x - 65536, x).to(torch.int16).view(torch.uint16))
        return out

    def dark_maps(density, seed, bits):
        """n maps: DNs in the lowest eighth of the range, a share `density` at 7/8 of it (threshold: 3/4)."""
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        top = 2 ** bits
        out = []
        for _ in range(n):
            x = torch.randint(0, top // 8, (H, W, C_), generator=gen, device=dev, dtype=torch.int32)
            if density > 0:
                x = torch.where(torch.rand((H, W, C_), generator=gen, device=dev) < density, torch.full_like(x, 7 * top // 8), x)
            out.append(x.to(torch.uint8) if bits == 8 else torch.where(x >= 32768, x - 65536, x).to(torch.int16).view(torch.uint16))
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
    icrf, diff = synthetic_icrf(bits=2 ** b)
    icrf8, diff8 = synthetic_icrf()
    stacks = [stack_u16(7 + 100 * s) for s in range(a.stacks)]
    stacks8, t8 = [], None
    for s in range(a.stacks):
        frames8, _, t8 = synthetic_stack_device(7 + 100 * s, n, H, W, device=dev)
        stacks8.append(frames8)
    kinds, info, hot_elements = {}, {}, {}
    for mode in ("val", "std"):
        std = mode == "std"
        plain = [engine.plan_merge(stacks[s], t, icrf, diff if std else None, stds[s] if std else None, bit_depth=b) for s in range(a.stacks)]
        kinds[f"u16_{mode}/no-maps"] = [p.launch for p in plain]
        info[f"u16_{mode}/no-maps"] = (plain[0].kernels, plain[0].algorithmic_bytes)
        plain[0].launch()
        for j, density in enumerate(densities):
            maps16, maps8 = dark_maps(density, 1000 + j, b), dark_maps(density, 1000 + j, 8)
            hot_elements[f"{density:g}"] = int(torch.stack([((m.view(torch.int16).to(torch.int32) & 0xFFFF) >= 3 * 2 ** (b - 2)) for m in maps16]).any(0).sum())
            plans = [engine.plan_merge(stacks[s], t, icrf, diff if std else None, stds[s] if std else None, darks=maps16,
                                       dark_min=[3 * 2 ** (b - 2)] * n, median_k=k, bit_depth=b) for s in range(a.stacks)]
            plans8 = [engine.plan_merge(stacks8[s], t8, icrf8, diff8 if std else None, stds[s] if std else None, darks=maps8, dark_min=[192] * n,
                                        median_k=k) for s in range(a.stacks)]
            if density == 0:                                        # nothing hot: hm_merge_u16's bits
                plans[0].launch()
                torch.cuda.synchronize()
                for q, o in plans[0].outputs.items():
                    assert torch.equal(o.view(torch.int64), plain[0].outputs[q].view(torch.int64)), (mode, q)
            kinds[f"u16_{mode}/d={density:g}"] = [p.launch for p in plans]
            info[f"u16_{mode}/d={density:g}"] = (plans[0].kernels, plans[0].algorithmic_bytes)
            kinds[f"u8_{mode}/d={density:g}"] = [p.launch for p in plans8]
            info[f"u8_{mode}/d={density:g}"] = (plans8[0].kernels, plans8[0].algorithmic_bytes)
    line = {"frames": n, "height": H, "width": W, "channels": C_, "bit_depth": b, "median_k": k, "steps": a.steps, "repeats": a.repeats,
            "resident_stacks": a.stacks, "device": torch.cuda.get_device_name(0), "hot_elements": hot_elements, "kinds": run_kinds(kinds, info)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
