#!/usr/bin/env python3
"""The all-pairs linearity statistics of a series that is resident as DN frames: the route through float64 frames against
engine.pairs_statistics_dn (hm_pairs_statistics_dn) in the same run, alternating.

7 frames, the 15 pairs with an exposure ratio >= 0.1 (exposures 2^i), 4096 x 4096 x 3, thresholds at 8 % / 90 % of the DN range, without
and with stds; uint8 frames, uint16 frames at 10 bits and at 12 bits. Kinds:
  a   N x linearize (with stds 2N: the std frame from the per-DN STD table, then value and std through ICRF and ICRF_diff) followed by
      pairs_statistics with thresholds - the route the DN entry replaces; its float64 frames are allocated by every call (torch's caching
      allocator, warm);
  b   pairs_statistics alone on float64 frames that are already resident (and already thresholded: the in-place step is idempotent);
  c   pairs_statistics_dn; where the depth's table fits in LDS, once per placement (variant 1: LDS, variant 2: global gathers), else the
      library's choice alone.
Times are host-clock microseconds per call around `--inner` back-to-back calls that end in one device synchronise, the median of `--reps`
such regions per kind, the kinds alternating region by region after one warm-up region of each; min and max beside it. Held bytes: what a
route keeps in device memory while it runs - DN frames, float64 frames, tables, workspace. c is checked against a bit for bit first.
--rehearse runs a tiny size on the HOST build to check the script itself; its times mean nothing."""
import argparse
import contextlib
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from camera_linearity_amd import _native as nat  # noqa: E402
from camera_linearity_amd import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=4096)
ap.add_argument("--frames", type=int, default=7)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--rehearse", action="store_true")
opt = ap.parse_args()

if opt.rehearse:
    dev, ctx = torch.device("cpu"), nat.host_mode()
    opt.size, opt.reps, opt.inner = 48, 2, 1
    print("REHEARSAL on the host build: the times below mean nothing")
else:
    assert torch.cuda.is_available(), "this benchmark measures the GPU: there is nothing to fall back to"
    dev, ctx = torch.device("cuda:0"), contextlib.nullcontext()
C_ = 3
H = opt.size


def sync():
    if dev.type == "cuda":
        torch.cuda.synchronize()


def tables(bits):
    rows = 2 ** bits
    x = np.arange(rows, dtype=np.float64) / (rows - 1)
    icrf = np.stack([x ** (1.0 + 0.35 * c) for c in range(C_)], axis=1)
    diff = np.stack([np.gradient(icrf[:, c], 2.0 / (rows - 1)) for c in range(C_)], axis=1) + 0.05
    k = np.arange(rows, dtype=np.float64)[:, None] * (256.0 / rows)
    std = 0.004 + 0.003 * np.sin(0.37 * k + np.arange(C_)[None, :]) ** 2
    thr = ([float(icrf[int(0.08 * rows), c]) for c in range(C_)], [float(icrf[int(0.90 * rows), c]) for c in range(C_)])
    return [torch.as_tensor(t, device=dev) for t in (icrf, diff, std)], thr


def make_frames(bits, n):
    """A near-linear camera: frame i = scene x t_i with 1 % noise, quantised to the depth."""
    g = torch.Generator(device=dev).manual_seed(4321 + bits)
    t = 2.0 ** np.arange(n)
    t /= t[-1]
    scene = 0.05 + 0.95 * torch.rand((H, H, C_), dtype=torch.float64, device=dev, generator=g)
    frames = []
    for ti in t:
        f = scene * float(ti) * (1 + 0.01 * torch.randn((H, H, C_), dtype=torch.float64, device=dev, generator=g))
        q = torch.clamp(torch.round(f * (2 ** bits - 1)), 0, 2 ** bits - 1)
        frames.append(q.to(torch.uint8) if bits == 8 else q.to(torch.int16).view(torch.uint16))     # (DNs below 2^15)
    pairs = [(i, j, float(t[i] / t[j])) for i in range(n) for j in range(n) if i < j and t[i] / t[j] >= 0.1]
    return frames, pairs


def held(*groups):
    return sum(t.numel() * t.element_size() for g in groups for t in g if t is not None)


def raw(stats):
    return torch.cat([d[k].reshape(-1) for ab, rel in stats for d in (ab, rel) for k in ("mean", "std", "error") if d[k] is not None]).view(torch.int64).cpu()


def show(ts):
    return f"{statistics.median(ts):9.1f} us (min {min(ts):.1f}, max {max(ts):.1f})"


with ctx:
    print(f"device: {torch.cuda.get_device_name(0) if dev.type == 'cuda' else 'host build'}; {opt.frames} frames of {H} x {H} x {C_}, "
          f"{opt.reps} regions of {opt.inner} calls per kind", flush=True)
    for bits in (8, 10, 12):
        (icrf, diff, std), thr = tables(bits)
        frames, pairs = make_frames(bits, opt.frames)
        bd = None if bits == 8 else bits
        E = H * H * C_
        for use_std in (False, True):
            def materialise():
                vals, stds = [], []
                for f in frames:
                    if use_std:
                        v, s = engine.linearize(f, engine.linearize(f, None, std, bit_depth=bd)[0], icrf, diff, bit_depth=bd)
                        stds.append(s)
                    else:
                        v = engine.linearize(f, None, icrf, bit_depth=bd)[0]
                    vals.append(v)
                return vals, (stds if use_std else None)

            vals, stds = materialise()
            kinds = {"a linearize + pairs_statistics": lambda: engine.pairs_statistics(*materialise(), pairs, thresholds=thr),
                     "b pairs_statistics, resident   ": lambda: engine.pairs_statistics(vals, stds, pairs, thresholds=thr)}
            args = (frames, pairs, icrf, diff if use_std else None, std if use_std else None)
            fits = "tab=lds" in engine.pairs_statistics_dn_kernel(E, opt.frames, len(pairs), C_, use_std, bits)
            for variant in ((1, 2) if fits else (0,)):
                name = engine.pairs_statistics_dn_kernel(E, opt.frames, len(pairs), C_, use_std, bits, variant)
                kinds[f"c pairs_statistics_dn {name}"] = (lambda v: lambda: engine.pairs_statistics_dn(*args, thresholds=thr, bit_depth=bd, variant=v))(variant)
            plan = engine.PairsDnPlan(*args, thr, bd, 0)
            bytes_a = held(frames, vals, stds or [])
            bytes_c = held(frames, plan.tables, [plan._ws, plan.outputs["stats"]])
            del plan
            results = {}
            for k, fn in kinds.items():                     # warm-up region of each kind; c against a, bit for bit
                for _ in range(opt.inner):
                    results[k] = fn()
                sync()
            ref = raw(results[next(iter(kinds))])
            same = all(torch.equal(raw(r), ref) for k, r in results.items() if k.startswith("c"))
            times = {k: [] for k in kinds}
            for _ in range(opt.reps):
                for k, fn in kinds.items():
                    sync()
                    t0 = time.perf_counter()
                    for _ in range(opt.inner):
                        fn()
                    sync()
                    times[k].append((time.perf_counter() - t0) * 1e6 / opt.inner)
            print(f"\n{'uint8' if bits == 8 else 'uint16'} {bits} bits, std {int(use_std)}, {len(pairs)} pairs: c {'equals' if same else 'DIFFERS FROM'} a bit for bit; "
                  f"held bytes a, b {bytes_a / 1e9:.3f} GB, c {bytes_c / 1e9:.3f} GB", flush=True)
            for k, ts in times.items():
                print(f"  {k:90s} {show(ts)}", flush=True)
            tb = times["b pairs_statistics, resident   "]
            print(f"  spread of b in this run: {max(tb) - min(tb):.1f} us", flush=True)
            del vals, stds, results
        del frames
        if dev.type == "cuda":
            torch.cuda.empty_cache()
