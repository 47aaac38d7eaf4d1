#!/usr/bin/env python3
"""Throughput of the noise-profile histogram (hm_noise_profile_update, csrc/hm_noise.hip): one launch = 32 device-resident uint8
frames against a uint8 mean frame, timed with HIP events, against its algorithmic bytes  E * (32 + 1) + 2 * 256 * 256 * C * 8.
Cases: 1920 x 1080 x 3 and 4096 x 4096 x 3 with sigma = 2 DN noise on a smooth scene (the mean is the scene's rounded value),
1920 x 1080 x 3 uniform-random DNs against a uniform-random mean (every element outside the LDS band: the global-atomic path),
and a constant frame (one bin takes every count). The host baseline is the reference as written: np.add.at over one
1920 x 1080 x 3 frame, channel by channel (video_processing.py:99-104), one thread.
Prints one JSON line. --quick: fewer repetitions and no pre-warm (profiling
runs); --case NAME: that case only, no host baseline."""
import ctypes
import json
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from camera_linearity_amd import _native as nat  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
QUICK = "--quick" in sys.argv
dev = torch.device("cuda:0")


def span(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def prewarm():
    x = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
    t0 = time.time()
    while time.time() - t0 < 0.5:
        x.add_(1)
    torch.cuda.synchronize()


def case(name, h, w, kind):
    g = torch.Generator(device=dev).manual_seed(7)
    C = 3
    if kind == "noise":
        yy = torch.linspace(0, 1, h, device=dev)[:, None, None]
        xx = torch.linspace(0, 1, w, device=dev)[None, :, None]
        scene = 255 * (0.5 * yy + 0.5 * xx) * torch.tensor([0.6, 0.8, 1.0], device=dev)
        mean = torch.round(scene).to(torch.uint8)
        frames = [torch.clamp(torch.round(scene + 2 * torch.randn((h, w, C), device=dev, generator=g)), 0, 255).to(torch.uint8)
                  for _ in range(nat.HM_MAX_FRAMES)]
        del scene
    elif kind == "uniform":
        mean = torch.randint(0, 256, (h, w, C), dtype=torch.uint8, device=dev, generator=g)
        frames = [torch.randint(0, 256, (h, w, C), dtype=torch.uint8, device=dev, generator=g) for _ in range(nat.HM_MAX_FRAMES)]
    else:
        mean = torch.full((h, w, C), 77, dtype=torch.uint8, device=dev)
        frames = [mean.clone() for _ in range(nat.HM_MAX_FRAMES)]
    n = h * w * C
    prof = torch.zeros((256, 256, C), dtype=torch.int64, device=dev)
    ptrs = (ctypes.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        nat.check(nat.hip_lib.hm_noise_profile_update(ptrs, len(frames), mean.data_ptr(), n, C, prof.data_ptr(), None, 0, stream))

    launch()
    torch.cuda.synchronize()
    assert int(prof.sum()) == len(frames) * n                  # every element counted once per frame
    iters, rounds = (3, 1) if QUICK else (20, 5)
    if not QUICK:                                              # (under a counter profiler every pre-warm kernel is serialised)
        prewarm()
    us = statistics.median(span(launch, iters) for _ in range(rounds))
    alg = nat.hip_lib.hm_noise_profile_algorithmic_bytes(len(frames), n, C)
    del frames
    torch.cuda.empty_cache()
    return {"case": name, "shape": [h, w, C], "frames_per_launch": nat.HM_MAX_FRAMES, "us_per_launch": round(us, 2),
            "algorithmic_bytes": alg, "gb_per_s": round(alg / us / 1e3, 1), "fraction_of_8TBps": round(alg / us / 1e-6 / HBM_BYTES_PER_S, 3)}


def host_baseline():
    """video_processing.py:99-104 as written, one 1920 x 1080 x 3 frame (np.add.at is single-threaded)."""
    rng = np.random.default_rng(1)
    mean = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    frame = np.clip(mean + np.around(rng.standard_normal(mean.shape) * 2), 0, 255).astype(np.uint8)
    prof = np.zeros((256, 256, 3), dtype=int)
    times = []
    for _ in range(1 if QUICK else 3):
        t0 = time.perf_counter()
        for c in range(3):
            np.add.at(prof[:, :, c], (mean[..., c].flatten(), frame[..., c].flatten()), 1)
        times.append(time.perf_counter() - t0)
    return {"s_per_frame": round(min(times), 4), "frames_per_s": round(1 / min(times), 2)}


def main():
    res = {"tool": "bench_noise_profile", "device": torch.cuda.get_device_name(0), "cases": []}
    only = sys.argv[sys.argv.index("--case") + 1] if "--case" in sys.argv else None
    for name, h, w, kind in (("1080p_sigma2", 1080, 1920, "noise"), ("4096_sigma2", 4096, 4096, "noise"),
                             ("1080p_uniform", 1080, 1920, "uniform"), ("1080p_constant", 1080, 1920, "constant")):
        if only is None or name == only:
            res["cases"].append(case(name, h, w, kind))
    if only is not None:
        print(json.dumps(res))
        return
    res["host_reference_np_add_at"] = host_baseline()
    gpu_fps = 32 / (res["cases"][0]["us_per_launch"] * 1e-6)
    res["speedup_1080p_vs_host_reference"] = round(gpu_fps / res["host_reference_np_add_at"]["frames_per_s"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
