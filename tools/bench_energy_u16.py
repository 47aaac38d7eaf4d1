#!/usr/bin/env python3
"""Where should a candidate's row live? hm_linearity_energy_u16's two placements - LDS (variant 1) and global gather (variant 2) - against
each other and against the 8-bit hm_linearity_energy on the same shapes, in ONE process on one MI355X.

Cells: 75 candidates on 28 x 28 x 7 (a stack thinned with data_spacing = 150), 256 x 256 x 7 and 1024 x 1024 x 7, and one lone candidate on
1024 x 1024 x 7 (the pair-major kernel); depths 10, 12, 14 and 16 with each variant that exists; with stds, relative. DNs are uniform over
the depth's range, the candidates power laws. The 8-bit entry on a stack of the same shape is the anchor, not a target.

Method: every kind of a cell (u8, lds, global) is recorded once as a hipGraph of `steps` back-to-back calls on preallocated buffers - the
entry points only enqueue kernels, so a graph holds exactly what a call launches, and no host time is measured with it. `steps` is chosen
per cell from one timed call so that a region lasts about --region-ms. After a pre-warm the kinds take turns, --repeats timed regions each
(HIP events around one replay); reported per kind: the median time per call and the spread (max - min) of the regions. Before anything is
timed the forced variants' out_energy and out_pairs are compared with the default's as bit patterns.

    python tools/bench_energy_u16.py [--log profiles/energy_u16_bench.log]

One JSON line per cell, then the table."""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

CELLS = [(28, 28, 7, 75), (256, 256, 7, 75), (1024, 1024, 7, 75), (1024, 1024, 7, 1)]      # (X, Y, N, candidates)
DEPTHS = [10, 12, 14, 16]
LDS_MAX_DEPTH = 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7, help="timed regions per kind (the kinds alternate)")
    ap.add_argument("--region-ms", type=float, default=30.0)
    ap.add_argument("--prewarm-s", type=float, default=0.3)
    ap.add_argument("--log", default=None, help="also write the output to this file")
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("at least 7 timed regions per kind")

    import numpy as np
    import torch
    from camera_linearity_amd import _native as nat
    from camera_linearity_amd import engine
    dev = torch.device("cuda", 0)
    lib = nat.hip_lib
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def problem(X, Y, N, B, depth, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        n = 2 ** depth
        dn = torch.randint(0, n, (X * Y, N), generator=g, device=dev, dtype=torch.int32)
        dn = dn.to(torch.uint8) if depth == 8 else dn.to(torch.int16).view(torch.uint16)       # (0 .. 65535 keep their low 16 bits)
        sd = 0.004 * (1 + torch.rand((X * Y, N), generator=g, device=dev, dtype=torch.float64))
        icrf = torch.linspace(0, 1, n, dtype=torch.float64, device=dev)[None, :] ** torch.linspace(1.5, 3.0, B, dtype=torch.float64, device=dev)[:, None]
        icrf[:, -1] = 1.0
        return dn.contiguous(), sd, icrf.contiguous(), int(0.02 * (n - 1)), int(0.98 * (n - 1))

    def caller(X, Y, N, B, depth, variant):
        """-> (a function that enqueues one call on the current stream, its outputs)"""
        dn, sd, icrf, lower, upper = problem(X, Y, N, B, depth, 11)
        P, pairs = X * Y, N * (N - 1) // 2
        t = (C.c_double * N)(*[1e-3 * 1.3 ** i for i in range(N)])
        energy = torch.empty(B, dtype=torch.float64, device=dev)
        out_pairs = torch.empty((B, pairs), dtype=torch.float64, device=dev)
        ws = torch.empty(lib.hm_linearity_energy_workspace_bytes(P, N, B) // 8, dtype=torch.float64, device=dev)
        keep = (dn, sd, icrf, t, ws)
        head = (dn.data_ptr(), sd.data_ptr(), t, icrf.data_ptr(), None, B, lower, upper, 1, P, N)
        tail = (out_pairs.data_ptr(), energy.data_ptr(), ws.data_ptr())

        def call():
            st = torch.cuda.current_stream(dev).cuda_stream
            rc = lib.hm_linearity_energy(*head, *tail, st) if depth == 8 else lib.hm_linearity_energy_u16(*head, depth, variant, *tail, st)
            assert rc == nat.HM_OK, rc
        call.keep = keep
        return call, (energy, out_pairs)

    def graph_of(call, steps):
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            call()                                               # (first launches load code objects and raise the LDS limit: outside the capture)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(steps):
                    call()
        torch.cuda.current_stream(dev).wait_stream(side)
        return g

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    say(f"# tools/bench_energy_u16.py on {torch.cuda.get_device_name(0)}: repeats={a.repeats} region-ms={a.region_ms}")
    table = []
    for X, Y, N, B in CELLS:
        u8_call, _ = caller(X, Y, N, B, 8, 0)
        u8_call()
        torch.cuda.synchronize()
        for depth in DEPTHS:
            kinds = {"u8": u8_call}
            default_call, default_out = caller(X, Y, N, B, depth, 0)
            default_call()
            want = [o.clone() for o in default_out]
            for name, v in (("lds", 1), ("global", 2)):
                if v == 1 and depth > LDS_MAX_DEPTH:
                    continue
                kinds[name], out = caller(X, Y, N, B, depth, v)
                kinds[name]()
                torch.cuda.synchronize()
                for got, ref in zip(out, want):                  # the placements and the default agree bit for bit
                    assert torch.equal(got.view(torch.int64), ref.view(torch.int64)), (X, Y, N, B, depth, name)
            torch.cuda.synchronize()
            one = max(timed(c) for c in kinds.values())
            steps = int(min(400, max(5, a.region_ms * 1e-3 / max(one, 1e-6))))
            graphs = {k: graph_of(c, steps) for k, c in kinds.items()}
            t_end = time.perf_counter() + a.prewarm_s
            while time.perf_counter() < t_end:
                for g in graphs.values():
                    g.replay()
                torch.cuda.synchronize()
            times = {k: [] for k in graphs}
            for _ in range(a.repeats):
                for k, g in graphs.items():
                    times[k].append(timed(g.replay) / steps)
            res = {k: dict(median_us=round(statistics.median(v) * 1e6, 2), spread_us=round((max(v) - min(v)) * 1e6, 2)) for k, v in times.items()}
            default = engine.energy_kernel(X * Y, N, B, True, depth, 0)
            say(json.dumps(dict(shape=[X, Y, N], candidates=B, bit_depth=depth, steps=steps, default=default, **res)))
            table.append((X, Y, N, B, depth, res, default))
    say("")
    say("| stack | candidates | bits | u8 anchor us | lds us (spread) | global us (spread) | default |")
    say("|---|---|---|---|---|---|---|")
    for X, Y, N, B, depth, res, default in table:
        cell = lambda k: f"{res[k]['median_us']} ({res[k]['spread_us']})" if k in res else "-"   # noqa: E731
        say(f"| {X} x {Y} x {N} | {B} | {depth} | {cell('u8')} | {cell('lds')} | {cell('global')} | {'lds' if 'lut=lds' in default else 'global'} |")
    if a.log:
        pathlib.Path(a.log).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.log).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
