#!/usr/bin/env python3
"""Where should hm_welford_update_u16 take a frame value from? Its placements - a table in LDS (variant 1), the computed quotient
(variant 2, no ICRF), the ICRF gathered from global memory (variant 3) - against each other and against the 8-bit hm_welford_update on
frames of the same shape, in ONE process on one MI355X.

Cells: 32 frames of 4096 x 4096 x 3 per launch, with m2; depths 10, 12, 14 and 16, with and without an ICRF, each placement that exists
for the cell. The uint16 DNs are uniform over all 16 bits (the kernels mask them to the depth), the ICRF a power law per channel. The 8-bit
entry on uint8 frames of the same shape is the anchor, not a target.

Method: a region is `steps` back-to-back launches on preallocated buffers between two HIP events (the entry points only enqueue a
kernel); `steps` is chosen per cell from one timed launch so that a region lasts about --region-ms. After a pre-warm the kinds take
turns, --repeats timed regions each; reported per kind: the median time per launch, the spread (max - min) of the regions, and the
fraction of 8 TB/s by hm_welford_u16_algorithmic_bytes (hm_welford_algorithmic_bytes for the anchor). Before anything is timed every forced
variant's mean and m2, from a zero state, are compared with the default's as bit patterns.

    python tools/bench_welford_u16.py [--log profiles/welford_u16_bench.log]

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

SHAPE, FRAMES = (4096, 4096, 3), 32
DEPTHS = [10, 12, 14, 16]
KINDS = (("lds", 1), ("computed", 2), ("global", 3))
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7, help="timed regions per kind (the kinds alternate)")
    ap.add_argument("--region-ms", type=float, default=30.0)
    ap.add_argument("--prewarm-s", type=float, default=0.3)
    ap.add_argument("--height", type=int, default=SHAPE[0], help="rows of a frame (smaller: a quick check of the tool)")
    ap.add_argument("--log", default=None, help="also write the output to this file")
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("at least 7 timed regions per kind")

    import torch
    from camera_linearity_amd import _native as nat
    from camera_linearity_amd import engine
    dev = torch.device("cuda", 0)
    lib = nat.hip_lib
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    shape = (a.height, SHAPE[1], SHAPE[2])
    n_elems, Cc = shape[0] * shape[1] * shape[2], shape[2]
    g = torch.Generator(device=dev).manual_seed(5)
    f16 = [torch.randint(0, 65536, shape, generator=g, device=dev, dtype=torch.int32).to(torch.int16).view(torch.uint16) for _ in range(FRAMES)]
    f8 = [torch.randint(0, 256, shape, generator=g, device=dev, dtype=torch.int32).to(torch.uint8) for _ in range(FRAMES)]
    p16, p8 = engine._ptr_array(f16), engine._ptr_array(f8)
    mean, m2 = (torch.zeros(shape, dtype=torch.float64, device=dev) for _ in range(2))
    gammas = torch.tensor([1.7, 2.0, 2.3], dtype=torch.float64, device=dev)[:Cc]

    def table(depth):
        rows = 256 if depth == 8 else 2 ** depth
        return (torch.linspace(0, 1, rows, dtype=torch.float64, device=dev)[:, None] ** gammas[None, :]).contiguous()

    def caller(depth, icrf, variant):
        """-> a function that enqueues one launch of 32 frames into mean / m2 (count_before = 32) on the current stream"""
        lut = None if icrf is None else icrf.data_ptr()

        def call(count_before=FRAMES):
            st = torch.cuda.current_stream(dev).cuda_stream
            head = (p8 if depth == 8 else p16, FRAMES, count_before, lut, mean.data_ptr(), m2.data_ptr(), n_elems, Cc)
            rc = lib.hm_welford_update(*head, st) if depth == 8 else lib.hm_welford_update_u16(*head, depth, variant, st)
            assert rc == nat.HM_OK, rc
        return call

    def state_of(call):
        mean.zero_()
        m2.zero_()
        call(0)
        torch.cuda.synchronize()
        return mean.view(torch.int64).clone(), m2.view(torch.int64).clone()

    def timed(fn, steps=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / steps

    say(f"# tools/bench_welford_u16.py on {torch.cuda.get_device_name(0)}: {FRAMES} frames of {shape[0]} x {shape[1]} x {shape[2]} per launch, "
        f"with m2; repeats={a.repeats} region-ms={a.region_ms}")
    bytes16 = lib.hm_welford_u16_algorithmic_bytes(FRAMES, 1, n_elems)
    bytes8 = lib.hm_welford_algorithmic_bytes(FRAMES, 1, n_elems)
    rows = []
    for with_icrf in (True, False):
        anchor = caller(8, table(8) if with_icrf else None, 0)
        for depth in DEPTHS:
            icrf = table(depth) if with_icrf else None
            default = engine.welford_kernel(n_elems, FRAMES, Cc, with_icrf, True, depth, 0)
            want = state_of(caller(depth, icrf, 0))
            kinds = {"u8": anchor}
            for name, v in KINDS:
                buf = C.create_string_buffer(64)
                if lib.hm_welford_update_u16_describe(n_elems, FRAMES, Cc, int(with_icrf), 1, depth, v, buf, len(buf)) != nat.HM_OK:
                    continue                                     # the placement does not exist for the cell, or its table does not fit
                kinds[name] = caller(depth, icrf, v)
                got = state_of(kinds[name])                      # the placements and the default agree bit for bit
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (depth, with_icrf, name)
            one = max(timed(c) for c in kinds.values())
            steps = int(min(400, max(3, a.region_ms * 1e-3 / max(one, 1e-6))))
            t_end = time.perf_counter() + a.prewarm_s
            while time.perf_counter() < t_end:
                for c in kinds.values():
                    c()
                torch.cuda.synchronize()
            times = {k: [] for k in kinds}
            for _ in range(a.repeats):
                for k, c in kinds.items():
                    times[k].append(timed(c, steps))
            res = {}
            for k, v in times.items():
                med = statistics.median(v)
                res[k] = dict(median_us=round(med * 1e6, 1), spread_us=round((max(v) - min(v)) * 1e6, 1),
                              of_peak=round((bytes8 if k == "u8" else bytes16) / med / PEAK, 3))
            say(json.dumps(dict(bit_depth=depth, icrf=with_icrf, steps=steps, default=default, **res)))
            rows.append((depth, with_icrf, res, default))
    say("")
    say("| bits | ICRF | u8 anchor us (spread) [of 8 TB/s] | lds | computed | global | default |")
    say("|---|---|---|---|---|---|---|")
    for depth, with_icrf, res, default in rows:
        cell = lambda k: f"{res[k]['median_us']} ({res[k]['spread_us']}) [{res[k]['of_peak']}]" if k in res else "-"   # noqa: E731
        say(f"| {depth} | {'yes' if with_icrf else 'no'} | {cell('u8')} | {cell('lds')} | {cell('computed')} | {cell('global')} | "
            f"{default.split('tab=')[1].split(',')[0]} |")
    if a.log:
        pathlib.Path(a.log).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.log).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
