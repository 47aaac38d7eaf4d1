#!/usr/bin/env python3
"""The distributions of all exposure pairs of a device-resident series: the fused call (engine.pairs_histogram -> hm_pairs_histogram)
against the existing per-pair path (compute_difference + two channel_histogram calls per pair) in the same run, alternating.

7 frames at exposures 2^i (the series' own pairs: the 15 with an exposure ratio >= 0.1), 1024 x 1024 x 3 and 4096 x 4096 x 3 float64,
bins 64 and 256, without and with stds, one fixed range for both kinds. Frames:
  linear   frame i = scene x t_i x (1 + 0.5 % noise): the absolute differences of a near-linear camera pile into a few bins around 0,
           so a wave's LDS atomics mostly hit the same address - the hot-bin case;
  spread   independent frames 0.5 +- 0.035 (uniform) compared with multiplier 1: both differences cover the range, the atomics spread
           over the bins. The gap between the two is what same-address serialisation costs.
Times are host-clock microseconds around calls that end in a device synchronise (both paths copy their histograms to the host), the
median of `--reps` alternating repetitions after one warm-up of each path; min and max are printed beside it. Bytes are algorithmic:
fused = every frame (and std) read once; per-pair = per pair 2 frames read, 2 difference images written and read back (x 2 with stds)."""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from camera_linearity_amd import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
ap.add_argument("--bins", type=int, nargs="+", default=[64, 256])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--frames", type=int, default=7)
opt = ap.parse_args()

assert torch.cuda.is_available(), "this benchmark measures the GPU: there is nothing to fall back to"
dev = torch.device("cuda:0")
RANGE = (-0.05, 0.05)
CHANNELS = [0, 1, 2]


def make(kind, n, H):
    g = torch.Generator(device=dev).manual_seed(1234 + H)
    t = 2.0 ** np.arange(n)
    t /= t[-1]
    scene = 0.1 + 0.8 * torch.rand((H, H, 3), dtype=torch.float64, device=dev, generator=g)
    frames, stds = [], []
    for ti in t:
        if kind == "linear":
            f = scene * float(ti) * (1 + 0.005 * torch.randn((H, H, 3), dtype=torch.float64, device=dev, generator=g))
        else:
            f = 0.5 + 0.035 * (2 * torch.rand((H, H, 3), dtype=torch.float64, device=dev, generator=g) - 1)
        frames.append(f)
        stds.append(0.002 + 0.01 * f.abs())
    pairs = [(i, j, float(t[i] / t[j]) if kind == "linear" else 1.0) for i in range(n) for j in range(n) if i < j and t[i] / t[j] >= 0.1]
    return frames, stds, pairs


def per_pair(frames, stds, pairs, bins):
    out = []
    for i, j, m in pairs:
        ad, ads, rd, rds = engine.compute_difference(frames[i], None if stds is None else stds[i], frames[j], None if stds is None else stds[j], m)
        out.append((engine.channel_histogram(ad, ads, bins, RANGE, CHANNELS), engine.channel_histogram(rd, rds, bins, RANGE, CHANNELS)))
        del ad, ads, rd, rds
    return out


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, res


def show(ts):
    return f"{statistics.median(ts):10.0f} us (min {min(ts):.0f}, max {max(ts):.0f})"


print(f"device: {torch.cuda.get_device_name(0)}; {opt.frames} frames, reps {opt.reps}", flush=True)
for H in opt.sizes:
    for kind in ("linear", "spread"):
        frames, stds_all, pairs = make(kind, opt.frames, H)
        E = H * H * 3
        for bins in opt.bins:
            for use_std in (False, True):
                stds = stds_all if use_std else None
                fused = lambda: engine.pairs_histogram(frames, stds, pairs, bins, RANGE, CHANNELS)       # noqa: E731
                loop = lambda: per_pair(frames, stds, pairs, bins)                                       # noqa: E731
                _, a = clock(fused)
                _, b = clock(loop)
                same = all(np.array_equal(x[k][c][0], y[k][c][0]) if not use_std else np.allclose(x[k][c][0], y[k][c][0], rtol=1e-9, atol=0)
                           for x, y in zip(a, b) for k in range(2) for c in CHANNELS)
                counted = sum(float(x[0][0][0].sum()) for x in a) / (len(pairs) * (E / 3)) if not use_std else float("nan")
                tf, tl = [], []
                for _ in range(opt.reps):
                    tf.append(clock(fused)[0])
                    tl.append(clock(loop)[0])
                s = 2 if use_std else 1
                bytes_f = opt.frames * s * 8 * E
                bytes_l = len(pairs) * 6 * s * 8 * E
                mf, ml = statistics.median(tf), statistics.median(tl)
                print(f"{H}x{H}x3 {kind:6s} bins {bins:4d} std {int(use_std)} pairs {len(pairs)}: fused {show(tf)} {bytes_f / mf / 1e6:7.3f} TB/s of {bytes_f / 1e9:.2f} GB"
                      f" | per-pair {show(tl)} {bytes_l / ml / 1e6:7.3f} TB/s of {bytes_l / 1e9:.2f} GB | per-pair / fused {ml / mf:5.2f}"
                      f" | results {'equal' if same else 'DIFFER'}; in range, channel 0 absolute: {counted:.3f}", flush=True)
        del frames, stds_all
        torch.cuda.empty_cache()
