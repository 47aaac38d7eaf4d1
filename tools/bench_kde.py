#!/usr/bin/env python3
"""Throughput of the weighted Gaussian KDE (hm_kde_moments + hm_kde_evaluate, csrc/hm_kde.hip) on 4096 x 4096 x 3 float64 data shaped like
a linearity difference image (normal, sigma 0.01 around small per-channel offsets), 1024 grid points per channel, all three channels,
without and with std (uniform in [0.002, 0.02]). Timed with HIP events: the moments of the three channels (two passes each) and the
evaluation of the three channels, separately. Reported per case:
  moments_us, evaluate_ms, pairs_per_s (counted elements x grid points / evaluate time),
  valu_per_pair (wave-level VALU instructions of k_kde_eval's inner loop per element-pair, from its ISA listing: 111 VALU, 96 of them
  FP64, per loop iteration of one element and 4 grid points per lane), and fraction_of_fp64_issue = the evaluate time the listing's
  instruction stream needs at 614.4 G wave-instructions/s (256 CU x 4 SIMD x 2.4 GHz / 4 cycles) over the measured time.
The host build (libhdrmerge_host.so, OpenMP) is timed on a 262 144-element subsample of one channel and extrapolated (labelled).
Prints one JSON line. --quick: fewer repetitions, no pre-warm, no host (profiling runs); --case nostd|std: that case only."""
import json
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from camera_linearity_amd import _native as nat, engine  # noqa: E402
from camera_linearity_amd.measurand import HostMeasurand  # noqa: E402

QUICK = "--quick" in sys.argv
ISSUE_RATE = 256 * 4 * 2.4e9 / 4                   # FP64 VALU wave-instructions per second
ISA_VALU_PER_PAIR = 111 / 4                         # k_kde_eval inner loop (hipcc -O3 -save-temps listing): per element x 4 points
ISA_F64_PER_PAIR = 96 / 4
H, W, C, M = 4096, 4096, 3, 1024
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
    while time.time() - t0 < 1.0:
        x.add_(1)
    torch.cuda.synchronize()


def data():
    g = torch.Generator(device=dev).manual_seed(11)
    val = torch.randn((H, W, C), dtype=torch.float64, device=dev, generator=g) * 0.01
    val += torch.tensor([0.0, 0.002, -0.001], dtype=torch.float64, device=dev)
    std = torch.rand((H, W, C), dtype=torch.float64, device=dev, generator=g) * 0.018 + 0.002
    return val, std


def case(name, val, std):
    n = val.numel()
    wsb = nat.hip_lib.hm_kde_workspace_bytes(n, C, M)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    mom = torch.empty((C, nat.HM_KDE_MOMENTS), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    sp = None if std is None else std.data_ptr()

    def moments():
        for c in range(C):
            nat.check(nat.hip_lib.hm_kde_moments(val.data_ptr(), sp, n, C, c, mom[c].data_ptr(), ws.data_ptr(), wsb, st))

    moments()
    momh = mom.cpu().numpy()
    params = [engine.kde_bandwidth(momh[c]) for c in range(C)]
    grid = torch.as_tensor(np.stack([np.linspace(p[2][0], p[2][1], M) for p in params]), device=dev)
    out = torch.empty((C, M), dtype=torch.float64, device=dev)

    def evaluate():
        for c in range(C):
            nat.check(nat.hip_lib.hm_kde_evaluate(val.data_ptr(), sp, n, C, c, params[c][0], params[c][1], grid[c].data_ptr(), M,
                                                  out[c].data_ptr(), ws.data_ptr(), wsb, st))

    evaluate()
    torch.cuda.synchronize()
    iters, rounds = (2, 1) if QUICK else (5, 3)
    if not QUICK:
        prewarm()
    mom_us = statistics.median(span(moments, iters * 4) for _ in range(rounds))
    ev_us = statistics.median(span(evaluate, iters) for _ in range(rounds))
    counted = float(momh[:, 0].sum())
    pairs = counted * M
    ideal_s = pairs * ISA_VALU_PER_PAIR / 64 / ISSUE_RATE
    res = {"case": name, "shape": [H, W, C], "data_points": M, "moments_us": round(mom_us, 1), "evaluate_ms": round(ev_us / 1e3, 3),
           "pairs": int(pairs), "pairs_per_s": float(f"{pairs / (ev_us * 1e-6):.4g}"), "valu_per_pair": ISA_VALU_PER_PAIR,
           "fp64_valu_per_pair": ISA_F64_PER_PAIR, "fraction_of_fp64_issue": round(ideal_s / (ev_us * 1e-6), 3),
           "integral": round(float(out.sum(1).mul(grid[:, 1] - grid[:, 0]).mean()), 6)}
    return res, (params, grid.cpu().numpy())


def host_extrapolated(val, std, params):
    """Host build on the first 262 144 elements of channel 0 at 1024 points, scaled to 4096 x 4096 x 3 (labelled as extrapolated)."""
    k = 1 << 18
    v = val[..., 0].reshape(-1)[:k].cpu().numpy().reshape(-1, 1).copy()
    s = None if std is None else std[..., 0].reshape(-1)[:k].cpu().numpy().reshape(-1, 1).copy()
    m = HostMeasurand(v, s)
    m.compute_kernel_density_estimate(M, channels=[0], use_std=s is not None)
    t0 = time.perf_counter()
    m.compute_kernel_density_estimate(M, channels=[0], use_std=s is not None)
    t = time.perf_counter() - t0
    return {"subsample_elements": k, "subsample_s": round(t, 3), "extrapolated_full_s": round(t * H * W * C / k, 1),
            "threads": torch.get_num_threads()}


def main():
    only = sys.argv[sys.argv.index("--case") + 1] if "--case" in sys.argv else None
    val, std = data()
    res = {"tool": "bench_kde", "device": torch.cuda.get_device_name(0), "cases": []}
    for name, s in (("nostd", None), ("std", std)):
        if only is None or name == only:
            r, (params, _) = case(name, val, s)
            if not QUICK:
                r["host_build_extrapolated"] = host_extrapolated(val, s, params)
            res["cases"].append(r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
