#!/usr/bin/env python3
"""Generate tests/golden/merge_describe_matrix.npz.xz: what hm_merge_describe / hm_merge_std_table_describe of the BUILT HIP library answer
for a full cross of call shapes - the library's own dispatch, run dry (fake aligned pointers, no device). The fixture pins the dispatch
across changes that must not move it (a re-layout of the merge sources, say): tests/test_merge_describe_matrix.py replays the matrix
on the library under test and compares return code and string of every entry.

The fixture is the project's own output, so it is only worth what the commit it was made at is worth: regenerate it at a commit whose
dispatch is known good (the parent of the change under test), never to make a failing replay pass.

Stored: the axes (JSON), every distinct string once (newline-joined bytes), and per entry a string index and the return code (entries in the axes' row-major order).

Usage:  python tests/golden/make_golden_describe.py        (writes tests/golden/merge_describe_matrix.npz.xz)
"""
import ctypes as C
import itertools
import json
import lzma
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
OUT = HERE / "merge_describe_matrix.npz.xz"

# the axes, slowest first. One entry of the matrix = one value of each.
AXES = {
    "n": list(range(1, 22)) + [24, 32, 33],
    "channels": [1, 2, 3, 4],
    "std": ["none", "frames", "table"],
    "flat": ["none", "u8", "f64"],
    "sum_w": [0, 1],
    "out_kind": [0, 1],
    "frames": ["u8", "f64"],
    "darks": ["none", "queue", "no_queue"],
    "align": ["aligned", "frame", "output"],          # one misaligned frame / the val output 8 bytes off a 16-byte boundary
    "shape": [[4, 8], [12, 44], [16, 64]],             # with C = 3: tail only, body plus tail, body only
    "variant": [0, -1, -2, 32],
}
N_MAX = max(AXES["n"])
BASE = 1 << 20
TABLE = BASE * 99


class Caller:
    """Builds one hm_merge_args per entry from fake pointers (allocated once) and asks the library to describe it."""

    def __init__(self, nat):
        self.nat = nat
        self.lib = nat.hip_lib
        ptrs = lambda vals: (C.c_void_p * N_MAX)(*vals)                                       # noqa: E731
        as_pp = lambda arr: C.cast(arr, C.POINTER(C.c_void_p))                                # noqa: E731
        self._keep = {
            "u8": ptrs([BASE * (i + 1) for i in range(N_MAX)]),
            "u8_off": ptrs([BASE * (i + 1) + (1 if i == 0 else 0) for i in range(N_MAX)]),     # frame 0 at an odd address
            "f64_off": ptrs([BASE * (i + 1) + (8 if i == 0 else 0) for i in range(N_MAX)]),    # frame 0 8-byte but not 16-byte aligned
            "sd": ptrs([BASE * (50 + i) for i in range(N_MAX)]),
            "dark": ptrs([BASE * 90] * N_MAX),
        }
        self.pp = {k: as_pp(v) for k, v in self._keep.items()}
        self._ex = (C.c_double * N_MAX)(*[1e-3 * 1.2 ** i for i in range(N_MAX)])
        self._dm = (C.c_int32 * N_MAX)(*[13] * N_MAX)
        self.buf = C.create_string_buffer(1024)

    def outer(self, n, channels, std, flat, sum_w, out_kind, frames):
        """The arguments the outer axes decide."""
        a = self.nat.MergeArgs()
        a.struct_size = C.sizeof(self.nat.MergeArgs)
        a.n_frames, a.channels, a.out_kind = n, channels, out_kind
        a.exposures = C.cast(self._ex, C.POINTER(C.c_double))
        a.icrf, a.w_lut = BASE * 40, BASE * 41
        if std != "none":
            a.icrf_diff, a.dw_lut, a.out_std = BASE * 43, BASE * 44, BASE * 45
            if std == "frames":
                a.stds = self.pp["sd"]
        if flat != "none":
            if flat == "u8":
                a.flat_u8 = BASE * 46
            else:
                a.flat_f64 = BASE * 46
            if std != "none":
                a.flat_std = BASE * 47
        if sum_w:
            a.out_sum_w = BASE * 48
        a.dark_min_dn = C.cast(self._dm, C.POINTER(C.c_int32))
        a.median_k = 3
        return a

    def inner(self, a, std, frames, darks, align, shape, variant):
        """The inner axes' fields (every one of them is rewritten on every call), then the dry dispatch."""
        H, W = shape
        a.height = a.rows = a.buf_rows = H
        a.width = W
        a.variant = variant
        fr = self.pp[("f64_off" if frames == "f64" else "u8_off") if align == "frame" else "u8"]
        if frames == "f64":
            a.frames_f64 = fr
        else:
            a.frames_u8 = fr
        a.out_val = BASE * 42 + (8 if align == "output" else 0)
        a.darks_u8 = self.pp["dark"] if darks != "none" else None
        a.hot_workspace = BASE * 91 if darks == "queue" else None
        a.hot_workspace_bytes = self.lib.hm_merge_hot_workspace_bytes(H * W * a.channels) if darks == "queue" else 0
        if std == "table":
            rc = self.lib.hm_merge_std_table_describe(C.byref(a), TABLE, C.addressof(self.buf), 1024)
        else:
            rc = self.lib.hm_merge_describe(C.byref(a), self.buf, 1024)
        return rc, self.buf.value


OUTER = ("n", "channels", "std", "flat", "sum_w", "out_kind", "frames")
INNER = ("darks", "align", "shape", "variant")
assert tuple(AXES) == OUTER + INNER


def replay(nat, axes):
    """(return code, string as bytes) of every entry of the matrix, in the stored (row-major) order."""
    call = Caller(nat)
    inner = list(itertools.product(*(axes[k] for k in INNER)))
    for o in itertools.product(*(axes[k] for k in OUTER)):
        a = call.outer(*o)
        std, frames = o[2], o[6]
        for i in inner:
            yield call.inner(a, std, frames, *i)


def main():
    sys.path.insert(0, str(HERE.parent.parent))
    from camera_linearity_amd import _native as nat
    strings, idx, rcs = {}, [], []
    for rc, s in replay(nat, AXES):
        idx.append(strings.setdefault(s, len(strings)))
        rcs.append(rc)
    names = sorted(strings, key=strings.get)
    with lzma.open(OUT, "wb", preset=9 | lzma.PRESET_EXTREME) as f:          # (xz: a third of the deflate of np.savez_compressed)
        np.savez(f, axes=np.array(json.dumps(AXES)), strings=np.frombuffer(b"\n".join(names), dtype=np.uint8),
                 index=np.asarray(idx, dtype=np.uint16 if len(names) < 65536 else np.uint32), rc=np.asarray(rcs, dtype=np.int8))
    print(f"{OUT.name}: {len(idx)} entries, {len(names)} distinct strings, {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
