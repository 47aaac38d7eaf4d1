#!/usr/bin/env python3
"""A handful of launches of merge_u16_stream per table placement, next to the uint8 kernels of the same shape, for rocprofv3 --pmc passes
(no pre-warm loop: counter collection serialises every dispatch). 7 x 2048 x 4096 x 3. usage: prof_merge_u16.py"""
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from camera_linearity_amd import engine  # noqa: E402
from camera_linearity_amd.synthetic import synthetic_exposures, synthetic_icrf, synthetic_stack_device  # noqa: E402

dev = torch.device("cuda:0")
n, H, W = 7, 2048, 4096
t = synthetic_exposures(n)
gen = torch.Generator(device=dev).manual_seed(7)
rad = torch.rand((H, W, 3), generator=gen, device=dev, dtype=torch.float64) * 4
stds = [torch.rand((H, W, 3), dtype=torch.float64, device=dev).mul_(0.004).add_(0.004) for _ in range(n)]
plans = []
for b, with_std in ((12, False), (10, True), (12, True), (16, False)):      # tab=lds, tab=lds, tab=mixed-wdwg, tab=global
    M = 2 ** b - 1
    k = M / (4 * t[n // 2])
    frames = []
    for ti in t:
        x = torch.clamp(torch.round(rad * float(ti * k)), 0, M).to(torch.int32)
        frames.append(torch.where(x >= 32768, x - 65536, x).to(torch.int16).view(torch.uint16))
    icrf, diff = synthetic_icrf(bits=2 ** b)
    plans.append(engine.plan_merge(frames, t, icrf, diff if with_std else None, stds if with_std else None, bit_depth=b))
frames8, _, t8 = synthetic_stack_device(7, n, H, W, device=dev)
icrf8, diff8 = synthetic_icrf()
plans += [engine.plan_merge(frames8, t8, icrf8), engine.plan_merge(frames8, t8, icrf8, diff8, stds)]
for p in plans:
    print(p.kernels)
    for _ in range(3):
        p.launch()
torch.cuda.synchronize()
print("done")
