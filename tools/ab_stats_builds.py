"""A/B of the weighted hm_channel_statistics and hm_axis_statistics (axis 0: thread kernel, axis 1: row kernel) on 4096 x 4096 x 3 between two
builds of libhdrmerge.so, loaded side by side with ctypes and timed with device events: two rounds, three timings of 30 launches each.
    python tools/ab_stats_builds.py BEFORE.so AFTER.so
profiles/stats_recentre_ab.log: the build before and after acc_add() re-centres a block on an overwhelming element."""
import ctypes as C
import sys

import torch

libs = {"before": C.CDLL(sys.argv[1]), "after": C.CDLL(sys.argv[2])}
torch.manual_seed(0)
dev = torch.device("cuda:0")
H = 4096
v = torch.rand(H, H, 3, dtype=torch.float64, device=dev)
s = 0.05 + 0.1 * torch.rand(H, H, 3, dtype=torch.float64, device=dev)
out = torch.empty(3 * H * 3 + 64, dtype=torch.float64, device=dev)
ws = torch.empty(1 << 22, dtype=torch.float64, device=dev)
vp = C.c_void_p
def timed(f, reps=30):
    for _ in range(5): f()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps): f()
        b.record(); torch.cuda.synchronize()
        best.append(a.elapsed_time(b) / reps * 1e3)
    return sorted(best)
for rnd in range(2):
    for name, lib in libs.items():
        lib.hm_axis_statistics_workspace_bytes.restype = C.c_size_t
        chan = lambda: lib.hm_channel_statistics(vp(v.data_ptr()), vp(s.data_ptr()), C.c_int64(v.numel()), 3, vp(out.data_ptr()), vp(ws.data_ptr()), None)
        ax0 = lambda: lib.hm_axis_statistics(vp(v.data_ptr()), vp(s.data_ptr()), C.c_int64(1), C.c_int64(H), C.c_int64(H * 3), vp(out.data_ptr()), vp(out.data_ptr() + 8 * H * 3), vp(out.data_ptr() + 16 * H * 3), vp(ws.data_ptr()), None)
        ax1 = lambda: lib.hm_axis_statistics(vp(v.data_ptr()), vp(s.data_ptr()), C.c_int64(H), C.c_int64(H), C.c_int64(3), vp(out.data_ptr()), vp(out.data_ptr() + 8 * H * 3), vp(out.data_ptr() + 16 * H * 3), vp(ws.data_ptr()), None)
        assert chan() == 0 and ax0() == 0 and ax1() == 0
        print(rnd, name, "channel us", [round(x, 1) for x in timed(chan)], "axis0 (thread) us", [round(x, 1) for x in timed(ax0)], "axis1 (row) us", [round(x, 1) for x in timed(ax1)], flush=True)
