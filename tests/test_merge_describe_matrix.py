"""The fused merge's dispatch, pinned: tests/golden/merge_describe_matrix.npz.xz holds what hm_merge_describe / hm_merge_std_table_describe
answered for a full cross of call shapes at the commit the fixture was made at (tests/golden/make_golden_describe.py: the axes, the
fake-pointer calls). The built library must answer the same - return code and string - for every entry: a change of the source layout
moves no call to another kernel. No GPU needed (the dispatch runs dry)."""
import importlib.util
import io
import json
import lzma
import pathlib
import re

import numpy as np

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"

FAMILIES = ["merge_u8_fast_std", "merge_u8_val3", "merge_u8_fast", "merge_u8_loop_std", "merge_u8_loop", "merge_f64_val", "merge_f64_std",
            "merge_generic", "merge_fixup_hot", "merge_patch_hot", "merge_scan_hot"]


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_describe", GOLDEN / "make_golden_describe.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_describe_matrix_replays_on_the_built_library():
    from camera_linearity_amd import _native as nat
    gen = _generator()
    z = np.load(io.BytesIO(lzma.open(GOLDEN / "merge_describe_matrix.npz.xz").read()))
    axes = json.loads(str(z["axes"]))
    strings = z["strings"].tobytes().split(b"\n")
    index, rcs = z["index"], z["rc"]
    n_entries = int(np.prod([len(v) for v in axes.values()]))
    assert len(index) == len(rcs) == n_entries

    # ---- the fixture covers every kernel family and every templated frame count (a fixture that misses one cannot pass)
    used = [strings[i].decode() for i in np.unique(index)]
    kernels = {k for s in used for k in s.split(" + ")}
    names = {re.match(r"[a-z0-9_]+", k).group(0) for k in kernels if k}
    for fam in FAMILIES:
        assert fam in names, fam
    # (the twelfth family, merge_u8_fast_std_lut, is described under merge_u8_fast_std's name with std=lut)
    for fam in ("merge_u8_val3", "merge_u8_fast", "merge_u8_fast_std"):
        have = {int(m.group(1)) for k in kernels for m in [re.match(re.escape(fam) + r"<N=(\d+),", k)] if m}
        assert have >= set(range(1, 21)), (fam, sorted(set(range(1, 21)) - have))
    lut = {int(m.group(1)) for k in kernels for m in [re.match(r"merge_u8_fast_std<N=(\d+),.*std=lut", k)] if m}
    assert lut >= set(range(1, 17)), sorted(set(range(1, 17)) - lut)

    # ---- the replay
    lookup = {s: i for i, s in enumerate(strings)}
    bad = []
    for e, (rc, s) in enumerate(gen.replay(nat, axes)):
        if rc != rcs[e] or lookup.get(s, -1) != index[e]:
            bad.append((e, int(rcs[e]), strings[index[e]].decode(), rc, s.decode()))
            if len(bad) >= 10:
                break
    assert e == n_entries - 1 or bad

    def where(e):
        out = {}
        for k in reversed(list(axes)):
            e, r = divmod(e, len(axes[k]))
            out[k] = axes[k][r]
        return dict(reversed(list(out.items())))
    assert not bad, "\n".join(f"{where(e)}: expected ({r0}, {s0!r}), got ({r1}, {s1!r})" for e, r0, s0, r1, s1 in bad)
