"""The argument rules of the TIFF, calibration, producer and all-pairs entries (csrc/hm_tiff_rules.h, hm_calibration_rules.h,
hm_producer_rules.h, hm_pairs_rules.h) and of the linearize, operator and pointwise entries (hm_frame_rules.h, hm_ops_rules.h) are written
once and compiled into both builds of the C ABI; the other per-frame entries, the correction entries and the single-pair / per-channel
statistics entries state theirs in each build. This sweep holds the two builds to the answers they always gave, for all of these entries,
in the manner of test_merge_rules_host.py: per entry point one base call that passes every rule, at the smallest shape that does so and on
real host arrays (the host build RUNS a call it accepts), every single fault applied to it, and every pair of faults whose codes differ - which pins the ORDER
of the rules. No GPU needed.

Every case asserts a literal status. The literals below - a fault's code and the place of its rule in the entry's order (`stage`: of two
faults in one call the lower stage answers) - were read off the libraries of the commit before the rules moved into the shared headers; they
are not derived from those headers. ALLOWED_DIFFERENCES lists the only faults the two builds may answer differently.

The device library never gets a call it could launch: every case sent to it carries a fault (or an early "nothing to do") of the device
build, and its whole half is skipped on a machine with a GPU - that the device build accepts valid calls is what the GPU suites of these
families show. tools/entry_rules_sweep.py prints the same sweep case by case for comparing two commits."""
import ctypes as C
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

OK, EINVAL, EUNSUP, EALIGN, ESHAPE = 0, -1, -2, -3, -6
NAN, INF = float("nan"), float("inf")
MAX_FRAMES, MAX_POP, MAX_PARAMS, MAX_PROBLEMS = 32, 1024, 32, 64
SAME = "same"


class Fault:
    """One change to a base call. `muts`: argument name (or "name[i]" for an entry of a per-frame / per-problem / per-pair array) -> the new
    value, or a function of the old one. dev / host: (code, stage) in that build, None where the change is no fault there (the call stays
    valid). unless: names of changes that make this one harmless. huge: the changed call is valid but far too large to run."""

    def __init__(self, name, muts, code=None, stage=None, *, host=SAME, unless=(), host_unless=(), huge=False):
        self.name, self.muts, self.unless, self.huge = name, muts, unless, huge
        self.host_unless = tuple(unless) + tuple(host_unless)           # changes that make this one harmless in the host build only
        self.dev = None if code is None else (code, stage)
        self.host = self.dev if host is SAME else host
        self.keys = {k.split("[")[0] for k in muts}

    def codes(self):
        return (self.dev and self.dev[0], self.host and self.host[0])


def null(*names, code=EINVAL, stage):
    return [Fault(f"{n}=NULL", {n: None}, code, stage) for n in names]


def vals(name, values, code, stage, **kw):
    return [Fault(f"{name}={v}", {name: v}, code, stage, **kw) for v in values]


def buf(n, dtype=np.float64, fill=0):
    """a 64-byte-aligned host array of n elements (kept alive by the caller)"""
    raw = np.zeros(n * np.dtype(dtype).itemsize + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    a = raw[off:off + n * np.dtype(dtype).itemsize].view(dtype)
    a[:] = fill
    return a


def ptr(a):
    return a.ctypes.data


def ptr_array(n, target):
    return (C.c_void_p * n)(*[target] * n)


class Entry:
    """An entry point's base call: `args` in the order of the C signature without the stream (ints, floats, addresses, ctypes arrays)."""

    def __init__(self, cid, fn, make, faults):
        self.cid, self.fn, self.make, self.faults = cid, fn, make, faults

    def call(self, lib, faults):
        args, keep = self.make()
        for f in faults:
            for key, value in f.muts.items():
                name, _, idx = key.partition("[")
                if idx:
                    arr, i = args[name], int(idx[:-1])
                    arr[i] = value(arr[i]) if callable(value) else value
                else:
                    args[name] = value(args[name]) if callable(value) else value
        rc = getattr(lib, self.fn)(*args.values(), None)
        del keep
        return rc


def expected(faults, build):
    """-> the literal status of a call with these faults in `build` ("dev" / "host"), None when none of them is a fault there"""
    names = {f.name for f in faults}
    live = [getattr(f, build) for f in faults if getattr(f, build) is not None and not names & set(f.host_unless if build == "host" else f.unless)]
    return min(live, key=lambda cs: cs[1])[0] if live else None


def _nat():
    from camera_linearity_amd import _native as nat
    return nat


# ---- the base calls ---------------------------------------------------------------------------------------------------------------------
def _stack():
    """2 frames of 12 elements (C = 3); the per-frame array has room for HM_MAX_FRAMES + 1 entries, all valid"""
    frame = buf(12, np.uint8, 7)
    return frame, ptr_array(MAX_FRAMES + 1, ptr(frame))


def make_welford_update():
    frame, frames = _stack()
    mean, m2 = buf(12), buf(12)
    return dict(frames=frames, n_frames=2, count_before=0, icrf=None, mean=ptr(mean), m2=ptr(m2), n_elems=12, C=3), (frame, mean, m2)


def make_welford_finalize():
    mean, m2, om, os_ = buf(12), buf(12), buf(12, np.uint8), buf(12, np.uint8)
    return dict(mean=ptr(mean), m2=ptr(m2), count=2, out_mean=ptr(om), out_std=ptr(os_), n_elems=12), (mean, m2, om, os_)


def make_noise_update():
    frame, frames = _stack()
    mean, prof = buf(12, np.uint8, 9), buf(256 * 256 * 3, np.int64)
    return dict(frames=frames, n_frames=2, mean=ptr(mean), n_elems=12, C=3, profiles=ptr(prof), workspace=None, workspace_bytes=0), (frame, mean, prof)


def make_noise_std():
    prof, edges, out = buf(256 * 256 * 3, np.int64, 1), buf(256), buf(256 * 3)
    return dict(profiles=ptr(prof), C=3, edges=ptr(edges), out_std=ptr(out)), (prof, edges, out)


def make_noise_clean():
    prof = buf(256 * 256 * 3, np.int64, 1)
    return dict(profiles=ptr(prof), C=3), (prof,)


def _kde_ws():
    n = _nat().hip_lib.hm_kde_workspace_bytes(12, 3, 4)
    return buf(n, np.uint8), n


def make_kde_moments():
    val, std, mom = buf(12, fill=0.5), buf(12, fill=1.0), buf(11)
    ws, n = _kde_ws()
    return dict(val=ptr(val), std=ptr(std), n_elems=12, C=3, channel=1, moments=ptr(mom), workspace=ptr(ws), workspace_bytes=n), (val, std, mom, ws)


def make_kde_evaluate():
    val, std, grid, out = buf(12, fill=0.5), buf(12, fill=1.0), buf(4, fill=0.25), buf(4)
    ws, n = _kde_ws()
    return dict(val=ptr(val), std=ptr(std), n_elems=12, C=3, channel=1, h=0.5, scale=1.0, grid=ptr(grid), m=4, out=ptr(out), workspace=ptr(ws),
                workspace_bytes=n), (val, std, grid, out, ws)


def _icrfs(rows):
    a = buf(rows * 256)
    a.reshape(rows, 256)[:] = np.linspace(0.0, 1.0, 256)
    return a


def _exposures():
    return (C.c_double * (MAX_FRAMES + 1))(*[1e-3 * 1.5 ** i for i in range(MAX_FRAMES + 1)])


def make_energy():
    """2 frames, 8 pixels, 2 candidates; dn and out_pairs have room for HM_MAX_FRAMES frames"""
    nat = _nat()
    dn, icrf = buf(8 * (MAX_FRAMES + 1), np.uint8, 100), _icrfs(2)
    out_pairs, out_energy = buf(2 * MAX_FRAMES * (MAX_FRAMES - 1) // 2), buf(2)
    ws = buf(nat.hip_lib.hm_linearity_energy_workspace_bytes(8, MAX_FRAMES, 2), np.uint8)
    ex = _exposures()
    return dict(dn=ptr(dn), std=None, exposures=ex, icrf=ptr(icrf), valid=None, n_candidates=2, lower=5, upper=250, use_relative=1, n_pixels=8,
                n_frames=2, out_pairs=ptr(out_pairs), out_energy=ptr(out_energy), workspace=ptr(ws)), (dn, icrf, out_pairs, out_energy, ws, ex)


def _de_state(K):
    """population 4, 1 parameter, 2 frames, 8 pixels, for K problems"""
    S, P = 4, 1
    a = dict(population=buf(K * S * P, fill=0.5), energies=buf(K * S), trial=buf(K * S * P), trial_energies=buf(K * S), icrf=buf(K * S * 256),
             valid=buf(K * S, np.uint8), status=buf(K * 8, np.int64), mean_icrf=_icrfs(K), pca=buf(K * 256 * P, fill=1e-3),
             lower_limits=buf(P, fill=-1.0), upper_limits=buf(P, fill=1.0))
    return a, {k: ptr(v) for k, v in a.items()}


def make_de():
    nat = _nat()
    keep, a = _de_state(1)
    dn, ex = buf(8 * (MAX_FRAMES + 1), np.uint8, 100), _exposures()
    ws = buf(nat.hip_lib.hm_de_workspace_bytes(8, MAX_FRAMES, 4), np.uint8)
    a.update(dn=ptr(dn), std=None, exposures=ex, n_pixels=8, n_frames=2, lower=5, upper=250, pop_size=4, n_params=1, seed=1, max_generations=10,
             mutation_lo=0.5, mutation_hi=1.0, recombination=0.7, tol=0.01, energy_limit=0.0, workspace=ptr(ws))
    return a, (keep, dn, ex, ws)


def make_de_batch():
    nat = _nat()
    keep, state = _de_state(2)
    dn, ex = buf(8 * (MAX_FRAMES + 1), np.uint8, 100), _exposures()
    ws = buf(nat.hip_lib.hm_de_batch_workspace_bytes(8, MAX_FRAMES, 4, 2), np.uint8)
    a = dict(n_problems=2, **state)
    a.update(dn=ptr_array(MAX_PROBLEMS + 1, ptr(dn)), std=None, seeds=(C.c_int64 * (MAX_PROBLEMS + 1))(*range(1, MAX_PROBLEMS + 2)), exposures=ex,
             n_pixels=8, n_frames=2, lower=5, upper=250, pop_size=4, n_params=1, max_generations=10, mutation_lo=0.5, mutation_hi=1.0,
             recombination=0.7, tol=0.01, energy_limit=0.0, workspace=ptr(ws))
    return a, (keep, dn, ex, ws)


def _pairs(out_len, ws_bytes):
    """2 frames, 1 pair, 12 elements (C = 3), with stds"""
    val, sd = buf(12, fill=0.5), buf(12, fill=0.1)
    out, ws = buf(out_len), buf(ws_bytes, np.uint8)
    a = dict(vals=ptr_array(MAX_FRAMES + 1, ptr(val)), stds=ptr_array(MAX_FRAMES + 1, ptr(sd)), n_frames=2, pair_i=(C.c_int32 * 2)(0, 0),
             pair_j=(C.c_int32 * 2)(1, 1), multipliers=(C.c_double * 2)(1.0, 1.0), n_pairs=1, n=12, C=3)
    return a, out, ws, (val, sd, out, ws)


def make_pairs_statistics():
    a, out, ws, keep = _pairs(18, _nat().hip_lib.hm_pairs_statistics_workspace_bytes(1))
    a.update(lower=None, upper=None, out=ptr(out), workspace=ptr(ws))
    return a, keep


def make_pairs_minmax():
    a, out, ws, keep = _pairs(12, _nat().hip_lib.hm_pairs_histogram_workspace_bytes(1, 4, 3))
    a.update(lower=None, upper=None, out=ptr(out), workspace=ptr(ws))
    return a, keep


def make_pairs_histogram():
    a, out, ws, keep = _pairs(2 * 3 * 4, _nat().hip_lib.hm_pairs_histogram_workspace_bytes(1, 4, 3))
    edges = buf(2 * 3 * 5)
    edges.reshape(6, 5)[:] = np.linspace(-1.0, 1.0, 5)
    a.update(channel_mask=7, lower=None, upper=None, edges=ptr(edges), bins=4, out=ptr(out), workspace=ptr(ws))
    return a, keep + (edges,)


def make_tiff_decode(compression):
    """a 4 x 4 x 3 uint8 image, 2 rows per strip: 2 strips of 24 bytes (for Compression 5 the bytes are no valid stream: the call is accepted
    and the strips' status words say so)"""
    def make():
        file, dst, status, ws = buf(48, np.uint8, 3), buf(48, np.uint8), buf(2, np.int64), buf(48, np.uint8)
        off, cnt = buf(2, np.int64), buf(2, np.int64, 24)
        off[1] = 24
        return dict(file=ptr(file), file_len=48, strip_offsets=ptr(off), strip_counts=ptr(cnt), n_strips=2, compression=compression, predictor=1,
                    rows_per_strip=2, height=4, width=4, samples=3, bytes_per_sample=1, color_mode=0, dst=ptr(dst), strip_status=ptr(status),
                    workspace=ptr(ws)), (file, dst, status, ws, off, cnt)
    return make


def make_tiff_encode(compression):
    """the same image written: src has room for float64 samples (src_kind 2)"""
    def make():
        lib = _nat().hip_lib
        cap = lib.hm_tiff_encode_payload_bytes(2, 24, compression)
        src, payload, off, cnt = buf(48, fill=0.5), buf(cap, np.uint8), buf(3, np.int64), buf(2, np.int64)
        ws = buf(max(16, lib.hm_tiff_encode_workspace_bytes(2, 24, 5)), np.uint8)
        return dict(src=ptr(src), src_kind=0, divisor=1.0, height=4, width=4, samples=3, rows_per_strip=2, compression=compression, predictor=1,
                    payload=ptr(payload), payload_cap=cap, strip_offsets=ptr(off), strip_counts=ptr(cnt), workspace=ptr(ws)), (src, payload, off, cnt, ws)
    return make


# ---- the faults: (code, stage) as the libraries before the shared headers answered ------------------------------------------------------
def frames_faults(name, n, stage, empty=("n_frames=0",)):
    return [Fault(f"{name}[{i}]=NULL", {f"{name}[{i}]": None}, EINVAL, stage, unless=empty) for i in range(n)]


def shift(by):
    return lambda p: p + by


DE_COMMON = (
    vals("pop_size", (3, 0, -1), EINVAL, 1) + vals("n_params", (0, -1), EINVAL, 1) + vals("n_pixels", (-1,), EINVAL, 1)
    + vals("max_generations", (-1,), EINVAL, 1)
    + vals("pop_size", (MAX_POP + 1,), ESHAPE, 2) + vals("n_params", (MAX_PARAMS + 1,), ESHAPE, 2)
    + vals("n_frames", (1, 0, -1, MAX_FRAMES + 1), ESHAPE, 3) + vals("n_frames", (MAX_FRAMES,), None, None)
    + vals("lower", (-1, 256), EINVAL, 5) + vals("upper", (-1, 256), EINVAL, 5)
    + vals("mutation_lo", (-0.1, 1.5, NAN), EINVAL, 6) + vals("mutation_hi", (2.0, NAN), EINVAL, 6)
    + vals("recombination", (-0.1, 1.1, NAN), EINVAL, 7) + vals("tol", (-1.0, NAN), EINVAL, 7) + vals("energy_limit", (NAN,), EINVAL, 7)
    + null("population", "energies", "trial", "trial_energies", "icrf", "valid", "status", stage=8)
    + null("mean_icrf", "pca", "lower_limits", "upper_limits", "dn", "exposures", stage=9)
    + [Fault("workspace=NULL", {"workspace": None}, EINVAL, 9, host=None)]
)


def _stop_flag(p):                                            # status[HM_DE_STOP] = 1 in the caller's status block
    C.cast(p, C.POINTER(C.c_int64))[2] = 1
    return p


PAIRS_COMMON = (
    null("vals", "pair_i", "pair_j", "multipliers", "out", "workspace", stage=1) + vals("n", (0, -1), EINVAL, 1) + vals("C", (0, 5), EINVAL, 1)
    + vals("n_frames", (0, -1, MAX_FRAMES + 1), EINVAL, 2) + vals("n_frames", (MAX_FRAMES,), None, None) + vals("n_pairs", (0, -1), EINVAL, 2)
    + vals("n", (11,), EINVAL, 2)
    + frames_faults("vals", 2, 3, empty=()) + frames_faults("stds", 2, 3, empty=())
    + [Fault("vals[1]+4", {"vals[1]": shift(4)}, EALIGN, 4), Fault("stds[0]+4", {"stds[0]": shift(4)}, EALIGN, 4), Fault("stds=NULL", {"stds": None})]
    + [Fault(f"{a}[0]={v}", {f"{a}[0]": v}, EINVAL, 5, unless=("n_frames=32",) if v == 2 else ())
       for a, v in (("pair_i", -1), ("pair_i", 2), ("pair_j", -1), ("pair_j", 2))]
)


def _limits(which):
    lim = (C.c_double * 3)(-10.0, -10.0, -10.0) if which == "lower" else (C.c_double * 3)(10.0, 10.0, 10.0)
    return Fault(f"{which} alone", {which: lim}, EINVAL, 2)


TIFF_DECODE = (
    null("file", "strip_offsets", "strip_counts", "dst", "strip_status", stage=1) + vals("file_len", (-1,), EINVAL, 1)
    + vals("n_strips", (0, -1), EINVAL, 2) + vals("rows_per_strip", (0,), EINVAL, 2) + vals("height", (0,), EINVAL, 2) + vals("width", (0,), EINVAL, 2)
    + vals("predictor", (0, 3), EINVAL, 3) + vals("color_mode", (-1, 2), EINVAL, 4)
    + vals("compression", (0, 2, 6), EUNSUP, 5) + vals("samples", (0, 2, 5), EUNSUP, 6) + vals("bytes_per_sample", (0, 2, 4), EUNSUP, 7)
    + [Fault("float64+predictor", {"bytes_per_sample": 8, "predictor": 2}, EUNSUP, 8),
       Fault("float64+color", {"bytes_per_sample": 8, "color_mode": 1}, EUNSUP, 8)]
    + vals("n_strips", (1, 3), ESHAPE, 9)
    # strip bytes = 2 rows x width x 1 sample: 2^31 is the largest strip the decoder takes
    + [Fault("strip=2^31", {"samples": 1, "width": 1 << 30}, huge=True), Fault("strip=2^31+2", {"samples": 1, "width": (1 << 30) + 1}, ESHAPE, 10)]
)

TIFF_ENCODE = (
    null("src", "payload", "strip_offsets", "strip_counts", stage=1)
    + vals("height", (0,), EINVAL, 2) + vals("width", (0,), EINVAL, 2) + vals("rows_per_strip", (0,), EINVAL, 2)
    + vals("predictor", (0, 3), EINVAL, 3) + vals("compression", (0, 2, 6), EUNSUP, 4) + vals("samples", (0, 2, 5), EUNSUP, 5)
    + vals("src_kind", (-1, 3), EUNSUP, 6)
    + [Fault(f"divisor={d}", {"src_kind": 2, "divisor": d}, EINVAL, 7) for d in (0.0, -1.0, NAN, INF)]
    + [Fault("src_kind=2", {"src_kind": 2}), Fault("float64+predictor", {"src_kind": 1, "predictor": 2}, EUNSUP, 8)]
    # strip bytes = 2 rows x width x 1 sample: 2^31 - 1 is the largest strip the encoder takes, so 2^31 - 2 is the largest of two rows
    + [Fault("strip=2^31-2", {"samples": 1, "width": (1 << 30) - 1, "payload_cap": 1 << 62}, huge=True),
       Fault("strip=2^31", {"samples": 1, "width": 1 << 30, "payload_cap": 1 << 62}, ESHAPE, 9)]
)
TIFF_ENCODE_TAIL = (
    [Fault("payload_cap=-1", {"payload_cap": -1}, ESHAPE, 11), Fault("payload_cap-1", {"payload_cap": lambda c: c - 1}, ESHAPE, 11)]
    + [Fault("payload+8", {"payload": shift(8)}, EALIGN, 12), Fault("strip_offsets+4", {"strip_offsets": shift(4)}, EALIGN, 12),
       Fault("strip_counts+4", {"strip_counts": shift(4)}, EALIGN, 12), Fault("src+4", {"src_kind": 2, "src": shift(4)}, EALIGN, 12)]
)

KDE_HEAD = (
    null("val", stage=1) + vals("n_elems", (-1,), EINVAL, 1) + vals("C", (0,), EINVAL, 1) + vals("channel", (-1, 3), EINVAL, 1)
    + vals("workspace_bytes", (-1,), EINVAL, 1) + [Fault("workspace=NULL", {"workspace": None}, EINVAL, 1, host=None)]
    + vals("n_elems", (11,), ESHAPE, 2) + [Fault("std=NULL", {"std": None})]
)

ENTRIES = [
    Entry("welford_update", "hm_welford_update", make_welford_update,
          vals("n_frames", (-1, MAX_FRAMES + 1), EINVAL, 1) + vals("count_before", (-1,), EINVAL, 1) + vals("n_elems", (-1,), EINVAL, 1)
          + vals("count_before", ((1 << 40) + 1,), EUNSUP, 2) + vals("count_before", (1 << 40,), None, None)
          + vals("C", (0, 5), ESHAPE, 3) + vals("n_elems", (11,), ESHAPE, 4) + vals("n_frames", (0,), OK, 5) + vals("n_elems", (0,), OK, 5)
          + null("frames", "mean", stage=6) + frames_faults("frames", 2, 7)
          + vals("n_frames", (MAX_FRAMES,), None, None) + [Fault("m2=NULL", {"m2": None})]),
    Entry("welford_finalize", "hm_welford_finalize", make_welford_finalize,
          vals("n_elems", (-1,), EINVAL, 1) + vals("count", (0, -1), EINVAL, 1) + vals("n_elems", (0,), OK, 2)
          + [Fault("mean=NULL", {"mean": None}, EINVAL, 3, unless=("out_mean=NULL",)), Fault("m2=NULL", {"m2": None}, EINVAL, 3, unless=("out_std=NULL",)),
             Fault("count=1", {"count": 1}, EINVAL, 4, unless=("out_std=NULL",)), Fault("out_mean=NULL", {"out_mean": None}),
             Fault("out_std=NULL", {"out_std": None})]),
    Entry("noise_profile_update", "hm_noise_profile_update", make_noise_update,
          vals("n_frames", (-1, MAX_FRAMES + 1), EINVAL, 1) + vals("n_elems", (-1,), EINVAL, 1) + vals("C", (0,), EINVAL, 1)
          + vals("workspace_bytes", (-1,), EINVAL, 1) + vals("C", (5,), EUNSUP, 2) + vals("n_elems", (11,), ESHAPE, 3)
          + null("frames", "mean", "profiles", stage=4) + frames_faults("frames", 2, 5)
          + vals("n_frames", (0,), OK, 6) + vals("n_elems", (0,), OK, 6) + vals("n_frames", (MAX_FRAMES,), None, None)),
    Entry("noise_profile_std", "hm_noise_profile_std", make_noise_std,
          null("profiles", "edges", "out_std", stage=1) + vals("C", (0, -1), EINVAL, 1) + vals("C", (5,), EUNSUP, 2)),
    Entry("noise_profile_clean_edges", "hm_noise_profile_clean_edges", make_noise_clean,
          null("profiles", stage=1) + vals("C", (0, -1), EINVAL, 1) + vals("C", (5,), EUNSUP, 2)),
    Entry("kde_moments", "hm_kde_moments", make_kde_moments,
          KDE_HEAD + [Fault("moments=NULL", {"moments": None}, EINVAL, 3, host=(EINVAL, 1)),
                      Fault("workspace_bytes=8", {"workspace_bytes": 8}, EINVAL, 3, host=None)]),
    Entry("kde_evaluate", "hm_kde_evaluate", make_kde_evaluate,
          KDE_HEAD + vals("m", (-1,), EINVAL, 3) + vals("h", (0.0, -1.0, NAN, INF), EINVAL, 3) + vals("scale", (NAN, INF), EINVAL, 3)
          + vals("m", (0,), OK, 4) + null("grid", "out", stage=5) + [Fault("workspace_bytes=8", {"workspace_bytes": 8}, EINVAL, 6, host=None)]),
    Entry("linearity_energy", "hm_linearity_energy", make_energy,
          vals("n_candidates", (-1,), EINVAL, 1) + vals("n_pixels", (-1,), EINVAL, 1) + vals("n_frames", (1, 0, -1, MAX_FRAMES + 1), ESHAPE, 2)
          + vals("lower", (-1, 256), EINVAL, 3) + vals("upper", (-1, 256), EINVAL, 3) + vals("n_candidates", (0,), OK, 4)
          + vals("n_candidates", (65536,), EUNSUP, 5) + [Fault("n_candidates=65535", {"n_candidates": 65535}, huge=True)]
          + null("dn", "exposures", "icrf", "out_energy", stage=6) + [Fault("workspace=NULL", {"workspace": None}, EINVAL, 6, host=None)]
          + vals("n_frames", (MAX_FRAMES,), None, None) + vals("n_pixels", (0,), None, None) + [Fault("out_pairs=NULL", {"out_pairs": None})]),
    Entry("de_generation", "hm_de_generation", make_de,
          DE_COMMON + [Fault("pop_size=1024", {"pop_size": MAX_POP}, huge=True), Fault("stop flag set", {"status": _stop_flag}, host=(OK, 10))]),
    Entry("de_generation_batch", "hm_de_generation_batch", make_de_batch,
          vals("n_problems", (0, -1), EINVAL, -2) + vals("n_problems", (MAX_PROBLEMS + 1,), ESHAPE, -1) + DE_COMMON
          + [Fault("64x1024 candidates", {"n_problems": MAX_PROBLEMS, "pop_size": MAX_POP}, EUNSUP, 4)]
          + null("seeds", stage=10) + frames_faults("dn", 2, 11, empty=())
          + [Fault("std[1]=NULL", {"std": lambda _: (C.c_void_p * 2)(1 << 20, None)}, EINVAL, 11)]),
    Entry("pairs_statistics", "hm_pairs_statistics", make_pairs_statistics,
          PAIRS_COMMON + [Fault("lower alone", {"lower": 1 << 20}, EINVAL, 2), Fault("upper alone", {"upper": 1 << 20}, EINVAL, 2)]),
    Entry("pairs_minmax", "hm_pairs_minmax", make_pairs_minmax, PAIRS_COMMON + [_limits("lower"), _limits("upper")]),
    Entry("pairs_histogram", "hm_pairs_histogram", make_pairs_histogram,
          PAIRS_COMMON + [_limits("lower"), _limits("upper")] + vals("bins", (0, -1, 2049), EINVAL, 6) + null("edges", stage=6)
          + vals("channel_mask", (-1, 8), EINVAL, 6)),
    Entry("tiff_decode/none", "hm_tiff_decode_strips", make_tiff_decode(1), TIFF_DECODE + [Fault("workspace=NULL", {"workspace": None})]),
    Entry("tiff_decode/lzw", "hm_tiff_decode_strips", make_tiff_decode(5), TIFF_DECODE + null("workspace", stage=11)),
    Entry("tiff_encode/none", "hm_tiff_encode_strips", make_tiff_encode(1),
          TIFF_ENCODE + TIFF_ENCODE_TAIL + [Fault("workspace=NULL", {"workspace": None}), Fault("workspace+8", {"workspace": shift(8)})]),
    Entry("tiff_encode/lzw", "hm_tiff_encode_strips", make_tiff_encode(5),
          TIFF_ENCODE + null("workspace", stage=10) + TIFF_ENCODE_TAIL + [Fault("workspace+8", {"workspace": shift(8)}, EALIGN, 12)]),
]

# ---- the per-frame, correction, operator, pointwise and single-pair / per-channel statistics entries -------------------------------------
# Base calls of 12 elements (C = 3) in buffers of 16, so that a pointer moved by half an element (a misalignment, which the host build mostly
# accepts and then runs) still addresses 12 elements of the test's own memory. (code, stage) as the libraries before hm_frame_rules.h and
# hm_ops_rules.h answered.
MAX_DIMS, TAKE_MAX, THR_MAX_CHANNELS = 6, 16, 32
SHARED = {"x": buf(16, fill=0.5), "x_u8": buf(16, np.uint8, 7), "map_f64": buf(16)}      # buffers a fault hands to a second argument


def dev_only(name, muts, code, stage, **kw):
    return Fault(name, muts, code, stage, host=None, **kw)


def misaligned(*names, stage, host=None, by=4):
    """pointers moved off their alignment: HM_EALIGN at `stage` in the device build (stage None: no alignment rule in either build)"""
    return [Fault(f"{n}+{by}", {n: shift(by)}, None if stage is None else EALIGN, stage, host=host) for n in names]


def f64s(*names, n=16, fill=0.5):
    keep = {k: buf(n, fill=fill) for k in names}
    return keep, {k: ptr(v) for k, v in keep.items()}


def make_u8_to_unit():
    dn, out = buf(16, np.uint8, 7), buf(16)
    return dict(dn=ptr(dn), out=ptr(out), n=12), (dn, out)


def make_weight_f64():
    keep, a = f64s("v", "w", "dw")
    return dict(a, n=12), keep


def make_weight_u8():
    dn = buf(16, np.uint8, 7)
    keep, a = f64s("w_lut", "dw_lut", n=256)
    keep2, b = f64s("w", "dw")
    return dict(dn=ptr(dn), **a, **b, n=12), (dn, keep, keep2)


def make_linearize(kind):
    """kind: "u8", "f64" or "u16" (9 bits); tables of 512 rows x 8 channels, so that C = 5 is a valid call where a build takes it"""
    def make():
        src = buf(16, {"u8": np.uint8, "f64": np.float64, "u16": np.uint16}[kind], 0.5 if kind == "f64" else 7)
        tabs, t = f64s("icrf", "icrf_diff", n=512 * 8)
        keep, a = f64s("std", "out_val", "out_std")
        idx = buf(16, np.uint16)
        args = {"v" if kind == "f64" else "dn": ptr(src), "std": a["std"], **t, "out_val": a["out_val"], "out_std": a["out_std"]}
        if kind != "u8":
            args["out_idx"] = ptr(idx)
        args.update(n=12, C=3, lut_stride=3)
        if kind == "u16":
            args["bit_depth"] = 9
        return args, (src, tabs, keep, idx)
    return make


def make_hot_filter(dtype):
    def make():
        x = SHARED["x_u8" if dtype is np.uint8 else "x"]
        m, out = buf(16, np.uint8, 1), buf(16, dtype)
        return dict(x=ptr(x), map_u8=ptr(m), map_f64=None, min_dn=200, thr=0.5, median_k=3, out=ptr(out), H=2, W=2, C=3), (m, out)
    return make


def make_roi_mean(dtype):
    def make():
        img, out = buf(32, dtype, 1), buf(4)
        ws = buf(_nat().hip_lib.hm_roi_mean_workspace_bytes(), np.uint8)
        return dict(img=ptr(img), H=2, W=3, C=3, x0=0, x1=2, y0=0, y1=3, out_mean=ptr(out), workspace=ptr(ws)), (img, out, ws)
    return make


def make_normalize():
    flat = buf(16, np.uint8, 200)
    keep, a = f64s("val", "std", "flat_std", "out_val", "out_std")
    return dict(val=a["val"], std=a["std"], flat_u8=ptr(flat), flat_f64=None, flat_std=a["flat_std"], ff_mean=(C.c_double * 4)(1, 1, 1, 1),
                ff_std_mean=(C.c_double * 4)(0.1, 0.1, 0.1, 0.1), out_val=a["out_val"], out_std=a["out_std"], n=12, C=3), (flat, keep)


def _dims(a, b, rest):
    """an int64 array of HM_MAX_DIMS + 1 entries: a, b, then `rest` (1 for extents, 0 for the strides of those extents)"""
    return (C.c_int64 * (MAX_DIMS + 1))(a, b, *[rest] * (MAX_DIMS - 1))


def make_binary_op():
    keep, a = f64s("x1", "s1", "x2", "s2", "out_val", "out_std")
    return dict(op=0, **a, ndim=2, shape=_dims(4, 3, 1), strides1=_dims(3, 1, 0), strides2=_dims(3, 1, 0)), keep


def make_unary_op():
    keep, a = f64s("x", "s", "out_val", "out_std")
    return dict(op=0, **a, n=12), keep


def make_pow_scalar():
    keep, a = f64s("x", "s", "out_val", "out_std")
    return dict(x=a["x"], s=a["s"], exponent=2.0, out_val=a["out_val"], out_std=a["out_std"], n=12), keep


def make_take_axis():
    """(2, 3, 2) -> three indices; the index array holds HM_TAKE_MAX + 1 valid entries, the outputs that many planes"""
    keep, a = f64s("x", "s")
    keep2, b = f64s("out_val", "out_std", n=128)
    return dict(**a, **b, outer=2, axis_len=3, inner=2, indices=(C.c_int64 * (TAKE_MAX + 1))(0, 2, -1), n_indices=3), (keep, keep2)


def make_thresholds():
    keep, a = f64s("val", "std")
    lim = lambda v: (C.c_double * (THR_MAX_CHANNELS + 1))(*[v] * (THR_MAX_CHANNELS + 1))   # noqa: E731
    return dict(**a, lower=lim(0.6), upper=lim(10.0), n=12, C=3), keep


def make_difference(bcast):
    def make():
        keep, a = f64s("x", "sx", "y", "sy", "out_abs", "out_abs_std", "out_rel", "out_rel_std")
        args = dict(x=a["x"], sx=a["sx"], y=a["y"], sy=a["sy"], multiplier=2.0, out_abs=a["out_abs"], out_abs_std=a["out_abs_std"],
                    out_rel=a["out_rel"], out_rel_std=a["out_rel_std"])
        args.update(dict(ndim=2, shape=_dims(4, 3, 1), strides_x=_dims(3, 1, 0), strides_y=_dims(3, 1, 0)) if bcast else dict(n=12))
        return args, keep
    return make


def make_interpolate(bcast):
    def make():
        keep, a = f64s("x0", "s0", "x1", "s1", "out", "out_std")
        args = dict(x0=a["x0"], s0=a["s0"], x1=a["x1"], s1=a["s1"], y0=0.0, y1=1.0, y=0.25, out=a["out"], out_std=a["out_std"])
        args.update(dict(ndim=2, shape=_dims(4, 3, 1), strides0=_dims(3, 1, 0), strides1=_dims(3, 1, 0)) if bcast else dict(n=12))
        return args, keep
    return make


def make_channel_statistics():
    keep, a = f64s("val", "std", "out")
    ws = buf(_nat().hip_lib.hm_channel_statistics_workspace_bytes(), np.uint8)
    return dict(val=a["val"], std=a["std"], n=12, C=3, out=a["out"], workspace=ptr(ws)), (keep, ws)


def make_pair_statistics():
    keep, a = f64s("x", "sx", "y", "sy")
    out, ws = buf(24), buf(_nat().hip_lib.hm_pair_statistics_workspace_bytes(), np.uint8)
    return dict(**a, multiplier=2.0, n=12, C=3, out=ptr(out), workspace=ptr(ws)), (keep, out, ws)


def make_axis_statistics():
    """(2, 2, 3); val and std hold the 192 elements of the (2, 32, 3) call whose axis the device build splits in two"""
    keep, a = f64s("val", "std", n=200)
    keep2, b = f64s("out_mean", "out_std", "out_err")
    ws = buf(max(64, _nat().hip_lib.hm_axis_statistics_workspace_bytes(2, 32, 3)), np.uint8)
    return dict(**a, outer=2, axis_len=2, inner=3, **b, workspace=ptr(ws)), (keep, keep2, ws)


def make_axis_statistics2():
    keep, a = f64s("val", "std")
    keep2, b = f64s("out_mean", "out_std", "out_err")
    ws = buf(max(64, _nat().hip_lib.hm_axis_statistics2_workspace_bytes(1, 2, 1, 2, 3)), np.uint8)
    return dict(**a, outer=1, a1=2, mid=1, a2=2, inner=3, **b, workspace=ptr(ws)), (keep, keep2, ws)


def _hist_ws():
    return buf(_nat().hip_lib.hm_histogram_workspace_bytes(4, 3), np.uint8)


def make_channel_minmax():
    keep, a = f64s("val", "std")
    out, ws = buf(8), _hist_ws()
    return dict(**a, n=12, C=3, out=ptr(out), workspace=ptr(ws)), (keep, out, ws)


def make_channel_histogram():
    """4 bins; edges and out have room for the largest histogram the ABI takes (bins * C = 8190)"""
    keep, a = f64s("val", "std")
    edges, out, ws = buf(2800), buf(8192), _hist_ws()
    edges[:5] = np.linspace(-1.0, 1.0, 5)
    return dict(**a, n=12, C=3, channel_mask=7, edges=ptr(edges), bins=4, lo=-1.0, hi=1.0, out=ptr(out), workspace=ptr(ws)), (keep, edges, out, ws)


def both_or_neither(out, ins, stage):
    """out_std with no std input, and std inputs with no out_std"""
    return [Fault(f"{out}=NULL", {out: None}, EINVAL, stage), Fault("no std input", {k: None for k in ins}, EINVAL, stage)]


N0 = ("n=0",)
LINEARIZE = (
    vals("n", (-1,), EINVAL, 1) + vals("C", (0,), EINVAL, 1) + [Fault("icrf=NULL", {"icrf": None}, EINVAL, 1, host=(EINVAL, 3))]
    + [Fault("out_val=NULL", {"out_val": None}, EINVAL, 1, unless=N0)] + vals("lut_stride", (2,), EINVAL, 2)
    + [dev_only("5 channels, 5 tables", {"C": 5, "lut_stride": 5}, EUNSUP, 3), Fault("5 channels, 1 table", {"C": 5, "lut_stride": 1}),
       Fault("n=0", {"n": 0}, OK, 4, host=(OK, 2)), Fault("std=NULL", {"std": None}), Fault("icrf_diff=NULL", {"icrf_diff": None})]
    + misaligned("out_val", "out_std", "std", stage=5)
)
LINEARIZE_U16 = (
    vals("n", (-1,), EINVAL, 1) + vals("C", (0,), EINVAL, 1) + null("icrf", stage=1)
    + [Fault(f"{k}=NULL", {k: None}, EINVAL, 1, unless=N0) for k in ("dn", "out_val")]
    + vals("lut_stride", (2,), EINVAL, 2) + vals("bit_depth", (8, 17), EINVAL, 2) + vals("bit_depth", (16,), None, None) + vals("n", (0,), OK, 3)
    + misaligned("out_val", "out_std", "std", stage=4, host=(EALIGN, 4)) + misaligned("dn", "out_idx", stage=4, host=(EALIGN, 4), by=1)
    + [Fault("std=NULL", {"std": None}), Fault("out_idx=NULL", {"out_idx": None})]
)


def hot_filter_faults(f64):
    return (vals("H", (-1,), EINVAL, 1) + vals("W", (-1,), EINVAL, 1) + vals("C", (0,), EINVAL, 1) + vals("H", (0,), OK, 2) + vals("W", (0,), OK, 2)
            + null("x", "out", stage=3) + [Fault("neither map", {"map_u8": None}, EINVAL, 3, unless=("both maps",)),
                                           Fault("both maps", {"map_f64": ptr(SHARED["map_f64"])}, host=(EINVAL, 3), unless=("neither map",)),
                                           dev_only("out=x", {"out": ptr(SHARED["x" if f64 else "x_u8"])}, EINVAL, 3, unless=("x+4",))]
            + vals("median_k", (1, 2, 4, 9), EINVAL, 4) + vals("median_k", (5, 7), None, None)
            + (misaligned("x", "out", stage=5) if f64 else []))


def roi_mean_faults(f64):
    return ((misaligned("img", stage=0) if f64 else []) + null("img", "out_mean", stage=1) + [dev_only("workspace=NULL", {"workspace": None}, EINVAL, 1)]
            + vals("C", (0, 5), EINVAL, 1) + vals("x0", (-1, 2), ESHAPE, 2) + vals("y0", (-1, 3), ESHAPE, 2) + vals("x1", (3, 0), ESHAPE, 2)
            + vals("y1", (4, 0), ESHAPE, 2))


def bcast_faults(s1, s2, stage):
    return (vals("ndim", (0, -1, MAX_DIMS + 1), EINVAL, stage) + vals("ndim", (1, MAX_DIMS), None, None) + null("shape", s1, s2, stage=stage))


def bcast_negatives(s1, s2, stage):
    return [Fault(f"{k}=-1", {k: -1}, EINVAL, stage, unless=("ndim=1",) if k.endswith("[1]") else ()) for k in ("shape[0]", "shape[1]", f"{s1}[0]", f"{s2}[1]")]


ELEMENTWISE = (
    vals("n", (-1,), EINVAL, 1) + vals("n", (0,), OK, 2) + null("x", "out_val", stage=3) + both_or_neither("out_std", ("s",), 3)
    + misaligned("x", "out_val", stage=4) + misaligned("s", "out_std", stage=None)
)
DIFFERENCE = (
    null("x", "y", "out_abs", "out_rel", stage=3) + null("out_abs_std", "out_rel_std", stage=4)
    + [Fault("no std input", {"sx": None, "sy": None}, EINVAL, 4), Fault("sx=NULL", {"sx": None}), Fault("sy=NULL", {"sy": None})]
    + misaligned("x", "y", "out_abs", "out_rel", stage=None)
)
INTERPOLATE = (
    null("x0", "x1", "out", stage=3) + both_or_neither("out_std", ("s0", "s1"), 3) + [Fault("s0=NULL", {"s0": None}), Fault("s1=NULL", {"s1": None})]
    + misaligned("x0", "x1", "out", stage=None)
)
COUNTS = vals("n", (0, -1), EINVAL, 1) + vals("C", (0, 5), EINVAL, 1)

ENTRIES += [
    Entry("u8_to_unit", "hm_u8_to_unit_f64", make_u8_to_unit,
          vals("n", (-1,), EINVAL, 1) + [Fault(f"{k}=NULL", {k: None}, EINVAL, 1, unless=N0) for k in ("dn", "out")] + vals("n", (0,), OK, 2)
          + misaligned("out", stage=3)),
    Entry("gaussian_weight_f64", "hm_gaussian_weight_f64", make_weight_f64,
          vals("n", (-1,), EINVAL, 1) + [Fault("v=NULL", {"v": None}, EINVAL, 1, unless=N0), dev_only("w=dw=NULL", {"w": None, "dw": None}, EINVAL, 1, unless=N0),
                                         Fault("w=NULL", {"w": None}), Fault("dw=NULL", {"dw": None})]
          + vals("n", (0,), OK, 2) + misaligned("v", "w", "dw", stage=3)),
    Entry("gaussian_weight_u8", "hm_gaussian_weight_u8", make_weight_u8,
          vals("n", (-1,), EINVAL, 1)
          + [Fault("dn=NULL", {"dn": None}, EINVAL, 1, unless=N0), Fault("w_lut=NULL", {"w_lut": None}, EINVAL, 1, unless=N0, host_unless=("w=NULL", "w=dw=NULL")),
             Fault("dw_lut=NULL", {"dw_lut": None}, EINVAL, 1, unless=N0 + ("dw=NULL",), host_unless=("w=dw=NULL",)), dev_only("w=dw=NULL", {"w": None, "dw": None}, EINVAL, 1, unless=N0),
             Fault("w=NULL", {"w": None}), Fault("dw=NULL", {"dw": None})]
          + vals("n", (0,), OK, 2) + misaligned("w", "dw", stage=3)),
    Entry("linearize_u8", "hm_linearize_u8", make_linearize("u8"), LINEARIZE + [Fault("dn=NULL", {"dn": None}, EINVAL, 1, unless=N0)]),
    Entry("linearize_f64", "hm_linearize_f64", make_linearize("f64"),
          LINEARIZE + [Fault("v=NULL", {"v": None}, EINVAL, 1, unless=N0), Fault("out_idx=NULL", {"out_idx": None})] + misaligned("v", stage=5)),
    Entry("linearize_u16", "hm_linearize_u16", make_linearize("u16"), LINEARIZE_U16),
    Entry("hot_pixel_filter_u8", "hm_hot_pixel_filter_u8", make_hot_filter(np.uint8), hot_filter_faults(False)),
    Entry("hot_pixel_filter_f64", "hm_hot_pixel_filter_f64", make_hot_filter(np.float64), hot_filter_faults(True)),
    Entry("roi_mean_u8", "hm_roi_mean_u8", make_roi_mean(np.uint8), roi_mean_faults(False)),
    Entry("roi_mean_f64", "hm_roi_mean_f64", make_roi_mean(np.float64), roi_mean_faults(True)),
    Entry("normalize_by_map", "hm_normalize_by_map", make_normalize,
          vals("n", (-1,), EINVAL, 1) + vals("C", (0, 5), EINVAL, 1) + vals("n", (0,), OK, 2) + null("val", "out_val", "ff_mean", stage=3)
          + [Fault("neither flat", {"flat_u8": None}, EINVAL, 3), Fault("both flats", {"flat_f64": ptr(SHARED["map_f64"])}, EINVAL, 3)]
          + [Fault(f"{k}=NULL", {k: None}, EINVAL, 4, unless=("out_std=NULL",)) for k in ("std", "flat_std", "ff_std_mean")]
          + [Fault("out_std=NULL", {"out_std": None})] + misaligned("val", "out_val", stage=None)),
    Entry("binary_op", "hm_binary_op", make_binary_op,
          vals("op", (-1, 5), EINVAL, 1) + vals("op", (4,), None, None) + bcast_faults("strides1", "strides2", 1) + null("x1", "x2", "out_val", stage=2)
          + both_or_neither("out_std", ("s1", "s2"), 3) + [Fault("s1=NULL", {"s1": None}), Fault("s2=NULL", {"s2": None})]
          + misaligned("x1", "x2", "out_val", stage=4) + misaligned("s1", "out_std", stage=None) + bcast_negatives("strides1", "strides2", 5)
          + [Fault("shape[0]=0", {"shape[0]": 0}, OK, 6)]),
    Entry("unary_op", "hm_unary_op", make_unary_op, vals("op", (-1, 3), EINVAL, 1) + vals("op", (2,), None, None) + ELEMENTWISE),
    Entry("pow_scalar", "hm_pow_scalar", make_pow_scalar, ELEMENTWISE + vals("exponent", (0.5, NAN), None, None)),
    Entry("take_axis", "hm_take_axis", make_take_axis,
          null("x", "out_val", "indices", stage=1) + vals("outer", (-1,), EINVAL, 1) + vals("axis_len", (0,), EINVAL, 1) + vals("inner", (0,), EINVAL, 1)
          + vals("n_indices", (0, -1), EINVAL, 1) + [dev_only("n_indices=17", {"n_indices": TAKE_MAX + 1}, EUNSUP, 2), Fault("n_indices=16", {"n_indices": TAKE_MAX})]
          + both_or_neither("out_std", ("s",), 3)
          + [Fault(f"indices[{i}]={v}", {f"indices[{i}]": v}, ESHAPE, 4) for i, v in ((0, 3), (1, -4), (2, 1 << 40))]
          # a refused call with the most indices an int counts must answer at once: no room for them is made before the rules have passed
          + [Fault("x=NULL, 2^31-1 indices", {"x": None, "n_indices": (1 << 31) - 1}, EINVAL, 1, huge=True)]
          + [Fault("indices[0]=-3", {"indices[0]": -3}), Fault("outer=0", {"outer": 0}, OK, 5)]),
    Entry("apply_thresholds", "hm_apply_thresholds", make_thresholds,
          vals("n", (-1,), EINVAL, 1) + vals("C", (0,), EINVAL, 1) + null("lower", "upper", stage=1) + vals("C", (THR_MAX_CHANNELS + 1,), EUNSUP, 2)
          + vals("C", (THR_MAX_CHANNELS, 5), None, None) + vals("n", (0,), OK, 3) + null("val", stage=4) + misaligned("val", "std", stage=5)
          + [Fault("std=NULL", {"std": None})]),
    Entry("compute_difference", "hm_compute_difference", make_difference(False), vals("n", (-1,), EINVAL, 1) + vals("n", (0,), OK, 2) + DIFFERENCE),
    Entry("interpolate", "hm_interpolate", make_interpolate(False), vals("n", (-1,), EINVAL, 1) + vals("n", (0,), OK, 2) + INTERPOLATE),
    Entry("compute_difference_bcast", "hm_compute_difference_bcast", make_difference(True),
          bcast_faults("strides_x", "strides_y", 1) + bcast_negatives("strides_x", "strides_y", 1) + [Fault("shape[0]=0", {"shape[0]": 0}, OK, 2)]
          + DIFFERENCE),
    Entry("interpolate_bcast", "hm_interpolate_bcast", make_interpolate(True),
          bcast_faults("strides0", "strides1", 1) + bcast_negatives("strides0", "strides1", 1) + [Fault("shape[0]=0", {"shape[0]": 0}, OK, 2)]
          + INTERPOLATE),
    Entry("channel_statistics", "hm_channel_statistics", make_channel_statistics,
          COUNTS + vals("n", (11,), EINVAL, 1) + null("val", "out", "workspace", stage=1) + misaligned("val", "std", stage=3, host=(EALIGN, 3))
          # more than 2^48 elements: the host build, which forwards to hm_axis_statistics, refuses them before it looks at the alignment
          + [Fault("n=3*2^49", {"n": 3 << 49}, host=(EINVAL, 2), huge=True), Fault("std=NULL", {"std": None})]),
    Entry("pair_statistics", "hm_pair_statistics", make_pair_statistics,
          COUNTS + vals("n", (11,), EINVAL, 1) + null("x", "y", "out", "workspace", stage=1)
          + misaligned("x", "y", "sx", "sy", stage=2, host=(EALIGN, 2)) + [Fault("sx=NULL", {"sx": None}), Fault("sy=NULL", {"sy": None})]),
    Entry("axis_statistics", "hm_axis_statistics", make_axis_statistics,
          vals("outer", (0,), EINVAL, 1) + vals("axis_len", (0, -1), EINVAL, 1) + vals("inner", (0,), EINVAL, 1)
          + [Fault("2^60 elements", {"outer": 1 << 20, "axis_len": 1 << 20, "inner": 1 << 20}, EINVAL, 1)] + null("val", "out_mean", "out_std", stage=1)
          + misaligned("val", "std", stage=2, host=(EALIGN, 2))
          + [dev_only("split axis, workspace=NULL", {"axis_len": 32, "workspace": None}, EINVAL, 3), Fault("split axis", {"axis_len": 32}),
             Fault("workspace=NULL", {"workspace": None}), Fault("std=NULL", {"std": None}), Fault("out_err=NULL", {"out_err": None})]),
    Entry("axis_statistics2", "hm_axis_statistics2", make_axis_statistics2,
          [Fault(f"{k}=0", {k: 0}, EINVAL, 1) for k in ("outer", "a1", "mid", "a2", "inner")]
          + [Fault("2^60 elements", {"outer": 1 << 20, "a1": 1 << 20, "a2": 1 << 20}, EINVAL, 1)] + null("val", "out_mean", "out_std", stage=1)
          + [dev_only("workspace=NULL", {"workspace": None}, EINVAL, 1)] + misaligned("val", "std", stage=2, host=(EALIGN, 2))
          + [Fault("std=NULL", {"std": None}), Fault("out_err=NULL", {"out_err": None})]),
    Entry("channel_minmax", "hm_channel_minmax", make_channel_minmax,
          COUNTS + null("val", "out", stage=1) + [dev_only("workspace=NULL", {"workspace": None}, EINVAL, 1), Fault("n=11", {"n": 11}),
                                                 Fault("std=NULL", {"std": None})] + misaligned("val", stage=None)),
    Entry("channel_histogram", "hm_channel_histogram", make_channel_histogram,
          COUNTS + vals("bins", (0, -1), EINVAL, 1) + null("val", "edges", "out", stage=1) + vals("hi", (-1.0, -2.0, NAN), EINVAL, 1)
          + [dev_only("workspace=NULL", {"workspace": None}, EINVAL, 1)] + vals("bins", (2731, 1 << 20), EUNSUP, 2) + vals("bins", (2730,), None, None)
          + [Fault("4 x 2048 bins", {"C": 4, "bins": 2048}), Fault("4 x 2049 bins", {"C": 4, "bins": 2049}, EUNSUP, 2), Fault("std=NULL", {"std": None})]),
]

# The only faults the two builds answer differently (the shared headers state each): the device build needs a workspace where the host
# build needs none, and checks its size; the host build, which does not ask for the workspace at that place, asks for hm_kde_moments'
# `moments` before the shape; on the host, where `status` is host memory, hm_de_generation reads the stop flag. Of the per-frame, correction,
# operator and statistics entries: the device build's alignment rules, workspaces and capacity refusals (five channels with five tables,
# 17 indices), and the rules the two builds word differently (a weight call with neither output, the hot-pixel filter's maps and x == out,
# linearize's table with no elements, the 2^48 elements that hm_channel_statistics takes on the host). This list grows only together
# with a line in the list of differences of a rule header or of DESIGN.md 4.5.
ALLOWED_DIFFERENCES = {
    ("kde_moments", "workspace=NULL"), ("kde_moments", "workspace_bytes=8"), ("kde_moments", "moments=NULL"),
    ("kde_evaluate", "workspace=NULL"), ("kde_evaluate", "workspace_bytes=8"),
    ("linearity_energy", "workspace=NULL"), ("de_generation", "workspace=NULL"), ("de_generation_batch", "workspace=NULL"),
    ("de_generation", "stop flag set"),
    ("u8_to_unit", "out+4"),
    ("gaussian_weight_f64", "v+4"), ("gaussian_weight_f64", "w+4"), ("gaussian_weight_f64", "dw+4"), ("gaussian_weight_f64", "w=dw=NULL"),
    ("gaussian_weight_u8", "w+4"), ("gaussian_weight_u8", "dw+4"), ("gaussian_weight_u8", "w=dw=NULL"),
    ("gaussian_weight_u8", "w_lut=NULL"), ("gaussian_weight_u8", "dw_lut=NULL"),       # (harmless on the host without `w` / without both outputs)
    ("linearize_u8", "icrf=NULL"), ("linearize_u8", "n=0"), ("linearize_u8", "5 channels, 5 tables"),
    ("linearize_u8", "out_val+4"), ("linearize_u8", "out_std+4"), ("linearize_u8", "std+4"),
    ("linearize_f64", "icrf=NULL"), ("linearize_f64", "n=0"), ("linearize_f64", "5 channels, 5 tables"),
    ("linearize_f64", "out_val+4"), ("linearize_f64", "out_std+4"), ("linearize_f64", "std+4"), ("linearize_f64", "v+4"),
    ("hot_pixel_filter_u8", "both maps"), ("hot_pixel_filter_u8", "out=x"),
    ("hot_pixel_filter_f64", "both maps"), ("hot_pixel_filter_f64", "out=x"), ("hot_pixel_filter_f64", "x+4"), ("hot_pixel_filter_f64", "out+4"),
    ("roi_mean_u8", "workspace=NULL"), ("roi_mean_f64", "workspace=NULL"), ("roi_mean_f64", "img+4"),
    ("binary_op", "x1+4"), ("binary_op", "x2+4"), ("binary_op", "out_val+4"), ("unary_op", "x+4"), ("unary_op", "out_val+4"),
    ("pow_scalar", "x+4"), ("pow_scalar", "out_val+4"), ("take_axis", "n_indices=17"), ("apply_thresholds", "val+4"), ("apply_thresholds", "std+4"),
    ("axis_statistics", "split axis, workspace=NULL"), ("axis_statistics2", "workspace=NULL"), ("channel_minmax", "workspace=NULL"),
    ("channel_histogram", "workspace=NULL"), ("channel_statistics", "n=3*2^49"),
}


def cases():
    """-> (id, entry, faults) of the whole sweep: the base call, every single fault, every pair of faults whose codes differ"""
    for e in ENTRIES:
        yield f"{e.cid}/base", e, ()
        for f in e.faults:
            yield f"{e.cid}/{f.name}", e, (f,)
        for f, g in itertools.combinations(e.faults, 2):
            if f.keys & g.keys or f.codes() == g.codes():
                continue
            yield f"{e.cid}/{f.name} & {g.name}", e, (f, g)


def sweep(dev_lib, host_lib):
    """-> (id, build, status or None where the case is not sent to that build, expected status). The host build gets a valid call only when
    it is small enough to run; the device build never gets one, and nothing at all where a GPU could run it."""
    use_device = dev_lib is not None and not torch.cuda.is_available()
    for cid, e, faults in cases():
        want_dev, want_host = expected(faults, "dev"), expected(faults, "host")
        rc_dev = e.call(dev_lib, faults) if use_device and want_dev is not None else None
        runs = want_host is None
        rc_host = None if runs and any(f.huge for f in faults) else e.call(host_lib, faults)
        yield cid, "device", rc_dev, want_dev
        yield cid, "host", rc_host, OK if runs else want_host


def test_differences_between_the_builds_are_the_listed_ones():
    differs = lambda f: f.dev != f.host or f.host_unless != tuple(f.unless)      # noqa: E731
    assert {(e.cid, f.name) for e in ENTRIES for f in e.faults if differs(f)} == ALLOWED_DIFFERENCES


def test_host_build_answers_as_before():
    nat = _nat()
    seen = set()
    for cid, build, rc, want in sweep(None, nat.host_lib()):
        if build == "host" and rc is not None:
            assert rc == want, (cid, rc, want)
            seen.add(rc)
    assert seen == {OK, EINVAL, EUNSUP, EALIGN, ESHAPE}         # the sweep reaches every status an argument can earn


@pytest.mark.skipif(torch.cuda.is_available(), reason="the device library is given host pointers: only where nothing can launch")
def test_device_build_answers_as_before_and_as_the_host_build():
    nat = _nat()
    sent, host_rc = 0, {}
    for cid, build, rc, want in sweep(nat.hip_lib, nat.host_lib()):
        if build == "device":
            if rc is None:
                continue
            assert want is not None and rc == want, (cid, rc, want)      # never a call without a device-build fault
            sent += 1
            host_rc[cid] = rc
        elif cid in host_rc and rc is not None:
            e_cid, _, names = cid.rpartition("/")
            if not any((e_cid, n) in ALLOWED_DIFFERENCES for n in names.split(" & ")):
                assert rc == host_rc[cid], (cid, host_rc[cid], rc)
    assert sent > 1000


def test_size_functions_agree_between_builds():
    nat = _nat()
    dev, host = nat.hip_lib, nat.host_lib()
    strips = (-1, 0, 1, 2, 3, (1 << 31) - 1)
    sizes = (-1, 0, 1, 15, 16, 17, 2047, 2048, (1 << 31) - 2, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, 1 << 40)
    for b in sizes:
        assert dev.hm_tiff_encode_bound(b) == host.hm_tiff_encode_bound(b), b
    assert dev.hm_tiff_encode_bound(0) == EINVAL and dev.hm_tiff_encode_bound(1 << 31) == ESHAPE and dev.hm_tiff_encode_bound((1 << 31) - 1) > 0
    for fn in ("hm_tiff_decode_workspace_bytes", "hm_tiff_encode_workspace_bytes", "hm_tiff_encode_payload_bytes"):
        for n, b, c in itertools.product(strips, sizes, (0, 1, 5, 6)):
            assert getattr(dev, fn)(n, b, c) == getattr(host, fn)(n, b, c), (fn, n, b, c)
    # decode takes a strip of 2^31 bytes, encode one byte less
    assert dev.hm_tiff_decode_workspace_bytes(1, 1 << 31, 5) == 1 << 31 and dev.hm_tiff_decode_workspace_bytes(1, (1 << 31) + 1, 5) == 0
    assert dev.hm_tiff_encode_payload_bytes(1, (1 << 31) - 1, 1) == (1 << 31) - 1 and dev.hm_tiff_encode_payload_bytes(1, 1 << 31, 1) == 0
