#!/usr/bin/env python3
"""The all-pairs linearity distributions of a series that is resident as DN frames: the route through float64 frames against
engine.pairs_histogram_dn (hm_pairs_histogram_dn) in the same process, alternating.

7 frames, the 15 pairs with an exposure ratio >= 0.1 (exposures 2^i), 4096 x 4096 x 3, thresholds at 8 % / 90 % of the DN range, a given
range (-0.05, 0.05) - so that every route is one histogram call, without the min / max pass - 64 and 256 bins, without and with stds;
uint8 frames and uint16 frames at 12 bits. Kinds:
  a   N x linearize (with stds 2N: the std frame from the per-DN STD table, then value and std through ICRF and ICRF_diff) followed by
      pairs_histogram with thresholds - the route the DN entry replaces; its float64 frames are allocated by every call (torch's caching
      allocator, warm);
  b   pairs_histogram alone on float64 frames that are already resident;
  c   pairs_histogram_dn, once per table placement the sizes admit (variant 1: LDS beside the histograms, variant 2: global gathers); the
      placement the library chooses (variant 0) is named beside them.
Every call ends in the engine's one device-to-host copy of the histograms, the same for every kind. Times are host-clock microseconds per
call around `--inner` back-to-back calls, the median of `--reps` such regions per kind, the kinds alternating region by region after one
warm-up region of each; min and max beside it. Held bytes: what a route keeps in device memory while it runs - DN frames, float64 frames,
tables, workspace, edges and histograms. Before timing c is compared with a: counts equal, a weighted bin within 2 (k + 2) u of its value
(k <= the pixels of a frame; the weights are positive).
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
ap.add_argument("--inner", type=int, default=5)
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
RANGE = (-0.05, 0.05)


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


def agrees(got, want, weighted):
    for g, w in zip(got, want):
        for gd, wd in zip(g, w):
            for c in wd:
                if not np.array_equal(gd[c][1], wd[c][1]):
                    return False
                if not weighted:
                    if not np.array_equal(gd[c][0], wd[c][0]):
                        return False
                elif np.any(np.abs(gd[c][0] - wd[c][0]) > 2 * (H * H + 2) * 2.0 ** -53 * np.abs(wd[c][0])):
                    return False
    return True


def show(ts):
    return f"{statistics.median(ts):9.1f} us (min {min(ts):.1f}, max {max(ts):.1f})"


with ctx:
    print(f"device: {torch.cuda.get_device_name(0) if dev.type == 'cuda' else 'host build'}; {opt.frames} frames of {H} x {H} x {C_}, "
          f"{opt.reps} regions of {opt.inner} calls per kind", flush=True)
    for bits in (8, 12):
        (icrf, diff, std), thr = tables(bits)
        frames, pairs = make_frames(bits, opt.frames)
        bd = None if bits == 8 else bits
        E, P = H * H * C_, len(pairs)
        chans = list(range(C_))
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
            for bins in (64, 256):
                kinds = {"a linearize + pairs_histogram": lambda: engine.pairs_histogram(*materialise(), pairs, bins, RANGE, chans, thresholds=thr),
                         "b pairs_histogram, resident   ": lambda: engine.pairs_histogram(vals, stds, pairs, bins, RANGE, chans, thresholds=thr)}
                args = (frames, pairs, icrf, diff if use_std else None, std if use_std else None)
                chosen = engine.pairs_histogram_dn_kernel(E, opt.frames, P, C_, use_std, bits, bins, 0)
                for variant in (1, 2):
                    try:
                        name = engine.pairs_histogram_dn_kernel(E, opt.frames, P, C_, use_std, bits, bins, variant)
                    except NotImplementedError:
                        continue                            # variant 1: not one pair's histograms fit beside the table
                    kinds[f"c pairs_histogram_dn variant {variant}: {name}"] = (lambda v: lambda: engine.pairs_histogram_dn(
                        *args, bins=bins, included_range=RANGE, channels=chans, thresholds=thr, bit_depth=bd, variant=v))(variant)
                out_bytes = P * 2 * C_ * (2 * bins + 1) * 8
                bytes_a = held(frames, vals, stds or []) + nat.lib.hm_pairs_histogram_workspace_bytes(P, bins, C_) + out_bytes
                bytes_c = (held(frames, [icrf, diff if use_std else None, std if use_std else None])
                           + nat.lib.hm_pairs_histogram_dn_workspace_bytes(P, bins, C_, bits) + out_bytes)
                results = {}
                for k, fn in kinds.items():                 # warm-up region of each kind; c against a
                    for _ in range(opt.inner):
                        results[k] = fn()
                    sync()
                ref = results[next(iter(kinds))]
                same = all(agrees(r, ref, use_std) for k, r in results.items() if k.startswith("c"))
                counted = sum(float(np.sum(d[c][0])) for ab, rel in ref for d in (ab, rel) for c in d)
                times = {k: [] for k in kinds}
                for _ in range(opt.reps):
                    for k, fn in kinds.items():
                        sync()
                        t0 = time.perf_counter()
                        for _ in range(opt.inner):
                            fn()
                        sync()
                        times[k].append((time.perf_counter() - t0) * 1e6 / opt.inner)
                print(f"\n{'uint8' if bits == 8 else 'uint16'} {bits} bits, std {int(use_std)}, {bins} bins, {P} pairs: c {'agrees with' if same else 'DIFFERS FROM'} a "
                      f"(sum of all bins {counted:.6g}); held bytes a, b {bytes_a / 1e9:.3f} GB, c {bytes_c / 1e9:.3f} GB; variant 0 runs {chosen}", flush=True)
                for k, ts in times.items():
                    print(f"  {k:120s} {show(ts)}", flush=True)
                tb = times["b pairs_histogram, resident   "]
                print(f"  spread of b in this run: {max(tb) - min(tb):.1f} us", flush=True)
                del results
            del vals, stds
        del frames
        if dev.type == "cuda":
            torch.cuda.empty_cache()
