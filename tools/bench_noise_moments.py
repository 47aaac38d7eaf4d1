#!/usr/bin/env python3
"""Throughput of the per-level noise moments of uint16 frames (hm_noise_moments_update_u16, csrc/hm_noise_u16.hip): one launch = 32
device-resident uint16 frames against a uint16 mean frame, timed with HIP events, against its algorithmic bytes
2 * E * (32 + 1) + 2 * 24 * 2^b * C (hm_noise_moments_algorithmic_bytes) and 8 TB/s.
Shapes 1920 x 1080 x 3 and 4096 x 4096 x 3; depths 10, 12 and 16 bits. Inputs: Gaussian noise of sigma = 2 / 255 of the DN range around a
photo-like mean (the mean frame is the scene's rounded value), and the same frames against a CONSTANT mean frame - every lane adds to the
same C levels: the contention case. Every placement that exists for a case is forced in turn (variant 1 = LDS where the table fits,
2 = global atomics, 3 = the LDS window) and the library's own choice is named. The anchor is the 8-bit hm_noise_profile_update on the same content at 255, in
the same process. Every launch is checked once: the counts must sum to frames * elements. Prints a line per timing and one JSON line at
the end. --quick: fewer repetitions and no pre-warm."""
import ctypes
import json
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from camera_linearity_amd import _native as nat  # noqa: E402
from camera_linearity_amd import engine  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
QUICK = "--quick" in sys.argv
FRAMES = nat.HM_MAX_FRAMES
C = 3
dev = torch.device("cuda:0")


def span(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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


def timed(launch):
    """median us per launch; the repetitions follow a first timed launch so that a slow (atomic-bound) case stays short"""
    launch()
    torch.cuda.synchronize()
    first = span(launch, 1)
    iters = 3 if QUICK else int(min(20, max(3, 2.0e5 / first)))
    return statistics.median(span(launch, iters) for _ in range(1 if QUICK else 3))


def content(h, w, max_dn):
    """32 frames of a photo-like scene in DNs of 0..max_dn with noise of sigma = 2 / 255 of the range, and the scene's rounded value"""
    g = torch.Generator(device=dev).manual_seed(7)
    yy = torch.linspace(0, 1, h, device=dev)[:, None, None]
    xx = torch.linspace(0, 1, w, device=dev)[None, :, None]
    scene = max_dn * (0.5 * yy + 0.5 * xx) * torch.tensor([0.6, 0.8, 1.0], device=dev)
    dtype = torch.uint8 if max_dn == 255 else torch.int32
    frames = [torch.clamp(torch.round(scene + (2 * max_dn / 255) * torch.randn((h, w, C), device=dev, generator=g)), 0, max_dn).to(dtype)
              for _ in range(FRAMES)]
    mean = torch.round(scene).to(dtype)
    if max_dn != 255:
        frames = [f.to(torch.int16).view(torch.uint16) for f in frames]
        mean = mean.to(torch.int16).view(torch.uint16)
    return frames, mean


def constant_like(mean, value):
    return torch.full(mean.shape, value, dtype=torch.int16 if mean.dtype == torch.uint16 else mean.dtype, device=dev).view(mean.dtype)


def moments_case(name, frames, mean, depth, variant, default_kernel):
    n = mean.numel()
    mom = torch.zeros((2 ** depth, C, 3), dtype=torch.int64, device=dev)
    ptrs = (ctypes.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        nat.check(nat.hip_lib.hm_noise_moments_update_u16(ptrs, len(frames), mean.data_ptr(), n, C, depth, mom.data_ptr(), variant, stream))

    launch()
    torch.cuda.synchronize()
    assert int(mom[:, :, 0].sum()) == len(frames) * n                  # every element counted once per frame
    us = timed(launch)
    alg = nat.hip_lib.hm_noise_moments_algorithmic_bytes(len(frames), n, C, depth)
    kernel = engine.noise_moments_kernel(n, len(frames), C, depth, variant)
    row = {"case": name, "bits": depth, "kernel": kernel, "library_choice": kernel == default_kernel, "us_per_launch": round(us, 2),
           "algorithmic_bytes": alg, "gb_per_s": round(alg / us / 1e3, 1), "fraction_of_8TBps": round(alg / us / 1e-6 / HBM_BYTES_PER_S, 3)}
    print(f"{name:28s} {kernel:44s} {'*' if row['library_choice'] else ' '} {us:12.2f} us  {row['gb_per_s']:8.1f} GB/s  "
          f"{row['fraction_of_8TBps']:.3f} of 8 TB/s", flush=True)
    return row


def anchor_case(name, frames, mean):
    n = mean.numel()
    prof = torch.zeros((256, 256, C), dtype=torch.int64, device=dev)
    ptrs = (ctypes.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        nat.check(nat.hip_lib.hm_noise_profile_update(ptrs, len(frames), mean.data_ptr(), n, C, prof.data_ptr(), None, 0, stream))

    launch()
    torch.cuda.synchronize()
    assert int(prof.sum()) == len(frames) * n
    us = timed(launch)
    alg = nat.hip_lib.hm_noise_profile_algorithmic_bytes(len(frames), n, C)
    print(f"{name:28s} {'k_noise_profile<C=3> (8-bit anchor)':44s}   {us:12.2f} us  {alg / us / 1e3:8.1f} GB/s  "
          f"{alg / us / 1e-6 / HBM_BYTES_PER_S:.3f} of 8 TB/s", flush=True)
    return {"case": name, "bits": 8, "kernel": "k_noise_profile<C=3>", "us_per_launch": round(us, 2), "algorithmic_bytes": alg,
            "gb_per_s": round(alg / us / 1e3, 1), "fraction_of_8TBps": round(alg / us / 1e-6 / HBM_BYTES_PER_S, 3)}


def main():
    res = {"tool": "bench_noise_moments", "device": torch.cuda.get_device_name(0), "frames_per_launch": FRAMES, "cases": []}
    if not QUICK:
        prewarm()
    for tag, h, w in (("1080p", 1080, 1920), ("4096", 4096, 4096)):
        frames, mean = content(h, w, 255)
        res["cases"].append(anchor_case(f"{tag}_noise", frames, mean))
        res["cases"].append(anchor_case(f"{tag}_constant_mean", frames, constant_like(mean, 77)))
        del frames, mean
        for depth in (10, 12, 16):
            max_dn = 2 ** depth - 1
            frames, mean = content(h, w, max_dn)
            n = mean.numel()
            default_kernel = engine.noise_moments_kernel(n, FRAMES, C, depth, 0)
            for kind, m in (("noise", mean), ("constant_mean", constant_like(mean, int(77 * max_dn / 255)))):
                for variant in (1, 2, 3):
                    try:
                        engine.noise_moments_kernel(n, FRAMES, C, depth, variant)
                    except NotImplementedError:                       # the table does not fit: the placement does not exist for the case
                        continue
                    res["cases"].append(moments_case(f"{tag}_{kind}", frames, m, depth, variant, default_kernel))
            del frames, mean
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
