#!/usr/bin/env python3
"""Print the output bits of the host build (libhdrmerge_host.so) for a fixed sweep of small calls: one line per call with its status and a
SHA-256 of every output buffer. Run it on two builds and diff the outputs to show that a change to the element formulas
(csrc/hm_*_math.h) or to hm_host.cpp's use of them moved no output bit:

    python tools/host_bits_sweep.py > this.txt
    HDRMERGE_HOST_LIB=<other>/libhdrmerge_host.so python tools/host_bits_sweep.py > other.txt

The host library is the only one called. Covered: the merge (all eight mode combinations of float64 / uint8 frames, dark maps and std
frames, plus the std-table, float32-std, uint16 and uint16-darks entries, with and without flat field, float64 and float32 outputs),
linearize, the Gaussian weight, normalize_by_map, the operators, difference and interpolate (dense and broadcast), the histograms and
min / max, welford_update and welford_update_u16 (with and without ICRF and m2, count_before 0 and 3, NaN and inf in the state, depths
9 / 12 / 16 with stray high bits), welford_finalize and welford_finalize_u16, noise_profile_clean_edges, the kernel density estimate
and differential-evolution generations.
Inputs are seeded and small (images of at most 9 x 11 x 3; N = 1, 2, 5); float inputs carry NaN, +-inf, +-0, negatives and values
outside [0, 1]. The hashes depend on the machine's libm: a before / after record, not a test fixture.
"""
import ctypes as C
import hashlib
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from camera_linearity_amd import _native as nat  # noqa: E402

L = nat.host_lib()
H, W, CH = 9, 11, 3
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -0.3, -1.0 / 255.0, 256.0 / 255.0, 1.7, 1e30, -1e30, 0.5, 1.0])


def p(a):
    return None if a is None else a.ctypes.data


def ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[p(a) for a in arrays])


def d3(*v):
    return (C.c_double * len(v))(*v)


def i64(*v):
    return (C.c_int64 * len(v))(*v)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def report(name, rc, **outs):
    print(f"{name:<64} rc={rc:<3} " + " ".join(f"{k}={sha(v)}" for k, v in outs.items() if v is not None))


def floats(rng, shape, specials=True, nan=True, lo=-0.2, hi=1.2):
    """Seeded float64 values, mostly inside [lo, hi], with the special values at fixed positions."""
    a = rng.uniform(lo, hi, size=shape)
    if specials:
        sp = SPECIALS if nan else SPECIALS[1:]
        flat = a.reshape(-1)
        step = max(1, flat.size // len(sp))
        for k, v in enumerate(sp):
            if k * step < flat.size:
                flat[k * step] = v
    return a


def stds_like(rng, shape, zeros=True):
    s = rng.uniform(1e-4, 0.05, size=shape)
    if zeros:
        s.reshape(-1)[::7] = 0.0
    return s


def tables(rng, rows, ch):
    icrf = np.sort(rng.uniform(0.0, 1.0, size=(rows, ch)), axis=0)
    icrf_diff = rng.uniform(0.5, 2.0, size=(rows, ch))
    return np.ascontiguousarray(icrf), icrf_diff


def weight_luts(bits):
    w, dw = (C.c_double * (1 << bits))(), (C.c_double * (1 << bits))()
    assert L.hm_gaussian_weight_lut_bits_host(bits, w, dw) == 0
    return np.array(w), np.array(dw)


# ---- the merge ----------------------------------------------------------------------------------------------------------------------
def merge_case(name, n, f64in=False, hot=False, std="none", flat="none", f32out=False, bits=0, k=3, seed=0):
    """std: none / f64 / table / f32; flat: none / u8 / f64; bits: 0 for the 8-bit entries, else the uint16 entries' bit depth."""
    rng = np.random.default_rng([seed, n, f64in, hot, bits])
    shape = (H, W, CH)
    rows = 1 << bits if bits else 256
    icrf, icrf_diff = tables(rng, rows, CH)
    w_lut, dw_lut = weight_luts(bits if bits else 8)
    keep = []
    a = nat.MergeArgs()
    a.struct_size = C.sizeof(nat.MergeArgs)
    a.n_frames, a.channels, a.height, a.width, a.rows, a.buf_rows = n, CH, H, W, H, H
    extra = []
    if bits:
        frames = [rng.integers(0, 1 << 16, size=shape, dtype=np.uint16) for _ in range(n)]
        extra.append(ptrs(frames))
    elif f64in:
        frames = [floats(rng, shape, nan=not hot) for _ in range(n)]
        a.frames_f64 = ptrs(frames)
    else:
        frames = [rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(n)]
        a.frames_u8 = ptrs(frames)
    keep += frames
    exposures = d3(*[0.01 * 2.0 ** i for i in range(n)])
    a.exposures = exposures
    a.icrf, a.icrf_diff, a.w_lut, a.dw_lut = p(icrf), p(icrf_diff), p(w_lut), p(dw_lut)
    with_std = std != "none"
    if std == "f64":
        sds = [stds_like(rng, shape, zeros=False) for _ in range(n)]
        a.stds = ptrs(sds)
        keep += sds
    elif std == "f32":
        sds = [stds_like(rng, shape, zeros=False).astype(np.float32) for _ in range(n)]
        extra.append(ptrs(sds))
        keep += sds
    elif std == "table":
        std_table = rng.uniform(1e-4, 0.05, size=(256, CH))
        extra.append(p(std_table))
    if hot:
        dt = np.uint16 if bits else np.uint8
        darks = [(rng.integers(0, 256, size=shape).astype(dt) if i % 2 == 0 else None) for i in range(n)]
        dmin = (C.c_int32 * n)(*[200 + i for i in range(n)])
        a.dark_min_dn, a.median_k = dmin, k
        if bits:
            extra.append(ptrs(darks))
        else:
            a.darks_u8 = ptrs(darks)
        keep += darks
    if flat == "u8":
        fu8 = rng.integers(1, 256, size=shape, dtype=np.uint8)
        a.flat_u8 = p(fu8)
    elif flat == "f64":
        ff = rng.uniform(0.2, 1.1, size=shape)
        a.flat_f64 = p(ff)
    if flat != "none":
        fstd = stds_like(rng, shape, zeros=False)
        a.flat_std = p(fstd)
        for c in range(CH):
            a.ff_mean[c], a.ff_std_mean[c] = 0.6 + 0.1 * c, 0.01 + 0.002 * c
    odt = np.float32 if f32out else np.float64
    a.out_kind = nat.HM_OUT_F32 if f32out else nat.HM_OUT_F64
    out_val, out_sum = np.full(shape, -7.0, odt), np.full(shape, -7.0)
    out_std = np.full(shape, -7.0, odt) if with_std else None
    a.out_val, a.out_std, a.out_sum_w = p(out_val), p(out_std), p(out_sum)
    if bits and hot:
        rc = L.hm_merge_u16_darks(C.byref(a), extra[0], extra[1], bits, None)
    elif bits:
        rc = L.hm_merge_u16(C.byref(a), extra[0], bits, None)
    elif std == "table":
        rc = L.hm_merge_std_table(C.byref(a), extra[0], None)
    elif std == "f32":
        rc = L.hm_merge_std_f32(C.byref(a), extra[0], None)
    else:
        rc = L.hm_merge(C.byref(a), None)
    report(name, rc, val=out_val, std=out_std, sum_w=out_sum)


def merge_sweep():
    for n in (1, 2, 5):
        for f64in in (False, True):
            for hot in (False, True):
                for std in ("none", "f64"):
                    for flat in ("none", "f64" if f64in else "u8"):
                        merge_case(f"merge n={n} f64in={int(f64in)} hot={int(hot)} std={std} flat={flat}", n, f64in, hot, std, flat)
                    merge_case(f"merge n={n} f64in={int(f64in)} hot={int(hot)} std={std} flat=f64 out=f32", n, f64in, hot, std, "f64", f32out=True)
        for f64in in (False, True):
            for hot in (False, True):
                for flat in ("none", "u8"):
                    for f32out in (False, True):
                        merge_case(f"merge_std_table n={n} f64in={int(f64in)} hot={int(hot)} flat={flat} f32={int(f32out)}", n, f64in, hot,
                                   "table", flat, f32out)
                        merge_case(f"merge_std_f32 n={n} f64in={int(f64in)} hot={int(hot)} flat={flat} f32={int(f32out)}", n, f64in, hot,
                                   "f32", flat, f32out)
        for bits in (10, 16):
            for hot in (False, True):
                for std in ("none", "f64"):
                    for flat in ("none", "f64"):
                        for f32out in (False, True):
                            merge_case(f"merge_u16 n={n} bits={bits} darks={int(hot)} std={std} flat={flat} f32={int(f32out)}", n, False, hot,
                                       std, flat, f32out, bits=bits)
    merge_case("merge n=5 f64in=1 hot=1 std=f64 flat=f64 k=5", 5, True, True, "f64", "f64", k=5)
    merge_case("merge n=5 f64in=0 hot=1 std=f64 flat=u8 k=7", 5, False, True, "f64", "u8", k=7)


# ---- linearize, weight, normalize --------------------------------------------------------------------------------------------------
def frame_sweep():
    rng = np.random.default_rng(11)
    n = H * W * CH
    icrf, icrf_diff = tables(rng, 256, CH)
    v, s = floats(rng, n), stds_like(rng, n)
    dn = rng.integers(0, 256, size=n, dtype=np.uint8)
    for stride, tabs in ((CH, (icrf, icrf_diff)), (1, (np.ascontiguousarray(icrf[:, 0]), np.ascontiguousarray(icrf_diff[:, 0])))):
        for with_std in (False, True):
            ov, os_, oi = np.full(n, -7.0), (np.full(n, -7.0) if with_std else None), np.full(n, 9, np.uint8)
            rc = L.hm_linearize_f64(p(v), p(s) if with_std else None, p(tabs[0]), p(tabs[1]) if with_std else None, p(ov), p(os_), p(oi), n, CH,
                                    stride, None)
            report(f"linearize_f64 stride={stride} std={int(with_std)}", rc, val=ov, std=os_, idx=oi)
            ov, os_ = np.full(n, -7.0), (np.full(n, -7.0) if with_std else None)
            rc = L.hm_linearize_u8(p(dn), p(s) if with_std else None, p(tabs[0]), p(tabs[1]) if with_std else None, p(ov), p(os_), n, CH, stride, None)
            report(f"linearize_u8 stride={stride} std={int(with_std)}", rc, val=ov, std=os_)
    for bits in (9, 12, 16):
        t16, d16 = tables(rng, 1 << bits, CH)
        dn16 = rng.integers(0, 1 << 16, size=n, dtype=np.uint16)
        ov, os_, oi = np.full(n, -7.0), np.full(n, -7.0), np.full(n, 9, np.uint16)
        rc = L.hm_linearize_u16(p(dn16), p(s), p(t16), p(d16), p(ov), p(os_), p(oi), n, CH, CH, bits, None)
        report(f"linearize_u16 bits={bits}", rc, val=ov, std=os_, idx=oi)
    w, dw = np.full(n, -7.0), np.full(n, -7.0)
    report("gaussian_weight_f64", L.hm_gaussian_weight_f64(p(v), p(w), p(dw), n, None), w=w, dw=dw)
    fine = np.linspace(-0.5, 1.5, 4001)
    w, dw = np.full(fine.size, -7.0), np.full(fine.size, -7.0)
    report("gaussian_weight_f64 ramp", L.hm_gaussian_weight_f64(p(fine), p(w), p(dw), fine.size, None), w=w, dw=dw)
    val, sd = floats(rng, n, lo=0.0, hi=3.0), stds_like(rng, n)
    fu8, ff, fs = rng.integers(0, 256, size=n, dtype=np.uint8), floats(rng, n, lo=0.1, hi=1.2), stds_like(rng, n)
    for kind in ("u8", "f64"):
        for with_std in (False, True):
            ov, os_ = np.full(n, -7.0), (np.full(n, -7.0) if with_std else None)
            rc = L.hm_normalize_by_map(p(val), p(sd) if with_std else None, p(fu8) if kind == "u8" else None, p(ff) if kind == "f64" else None,
                                       p(fs) if with_std else None, d3(0.6, 0.7, 0.8, 0.0), d3(0.01, 0.02, 0.03, 0.0) if with_std else None,
                                       p(ov), p(os_), n, CH, None)
            report(f"normalize_by_map flat={kind} std={int(with_std)}", rc, val=ov, std=os_)


# ---- operators, difference, interpolate -------------------------------------------------------------------------------------------
def ops_sweep():
    rng = np.random.default_rng(23)
    shape = (H, W, CH)
    n = H * W * CH
    x1, x2 = floats(rng, shape, lo=-2.0, hi=3.0), floats(rng, shape, lo=-2.0, hi=3.0)[::-1].copy()
    s1, s2 = stds_like(rng, shape), stds_like(rng, shape)
    row, srow = floats(rng, (1, W, 1), lo=-2.0, hi=3.0), stds_like(rng, (1, W, 1))
    dense, bc = i64(W * CH, CH, 1), i64(0, 1, 0)
    sh = i64(H, W, CH)
    for op, name in enumerate(("add", "sub", "mul", "div", "pow")):
        for a_std, b_std in ((True, True), (True, False), (False, True), (False, False)):                  # out_std exactly when an operand has one
            want = a_std or b_std
            for second, s_second, st2, tag in ((x2, s2, dense, "dense"), (row, srow, bc, "bcast")):
                ov, os_ = np.full(shape, -7.0), (np.full(shape, -7.0) if want else None)
                rc = L.hm_binary_op(op, p(x1), p(s1) if a_std else None, p(second), p(s_second) if b_std else None, p(ov), p(os_), 3, sh, dense,
                                    st2, None)
                report(f"binary_op {name} {tag} s1={int(a_std)} s2={int(b_std)} out_std={int(want)}", rc, val=ov, std=os_)
    flat1, sflat1 = x1.reshape(-1), s1.reshape(-1)
    for op, name in enumerate(("neg", "log_e", "log_10")):
        for with_std in (False, True):
            ov, os_ = np.full(n, -7.0), (np.full(n, -7.0) if with_std else None)
            rc = L.hm_unary_op(op, p(flat1), p(sflat1) if with_std else None, p(ov), p(os_), n, None)
            report(f"unary_op {name} std={int(with_std)}", rc, val=ov, std=os_)
    for pw in (2.0, 0.5, 1.0, 3.0, -2.0, 1.7):
        for with_std in (False, True):
            ov, os_ = np.full(n, -7.0), (np.full(n, -7.0) if with_std else None)
            rc = L.hm_pow_scalar(p(flat1), p(sflat1) if with_std else None, pw, p(ov), p(os_), n, None)
            report(f"pow_scalar p={pw} std={int(with_std)}", rc, val=ov, std=os_)
    for sx, sy in ((False, False), (True, True), (True, False), (False, True)):
        std = sx or sy
        o = [np.full(shape, -7.0) if (std or k % 2 == 0) else None for k in range(4)]      # abs, abs_std, rel, rel_std
        rc = L.hm_compute_difference(p(x1), p(s1) if sx else None, p(x2), p(s2) if sy else None, 1.9, p(o[0]), p(o[1]), p(o[2]), p(o[3]), n, None)
        report(f"compute_difference sx={int(sx)} sy={int(sy)}", rc, abs=o[0], abs_std=o[1], rel=o[2], rel_std=o[3])
        o = [np.full(shape, -7.0) if (std or k % 2 == 0) else None for k in range(4)]
        rc = L.hm_compute_difference_bcast(p(x1), p(s1) if sx else None, p(row), p(srow) if sy else None, 0.37, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
                                           3, sh, dense, bc, None)
        report(f"compute_difference_bcast sx={int(sx)} sy={int(sy)}", rc, abs=o[0], abs_std=o[1], rel=o[2], rel_std=o[3])
        for want in (std,):
            ov, os_ = np.full(shape, -7.0), (np.full(shape, -7.0) if want else None)
            rc = L.hm_interpolate(p(x1), p(s1) if sx else None, p(x2), p(s2) if sy else None, 0.01, 0.08, 0.03, p(ov), p(os_), n, None)
            report(f"interpolate s0={int(sx)} s1={int(sy)} out_std={int(want)}", rc, val=ov, std=os_)
            ov, os_ = np.full(shape, -7.0), (np.full(shape, -7.0) if want else None)
            rc = L.hm_interpolate_bcast(p(x1), p(s1) if sx else None, p(row), p(srow) if sy else None, 0.01, 0.08, 0.03, p(ov), p(os_), 3, sh, dense,
                                        bc, None)
            report(f"interpolate_bcast s0={int(sx)} s1={int(sy)} out_std={int(want)}", rc, val=ov, std=os_)


# ---- histograms and min / max ----------------------------------------------------------------------------------------------------
def stats_sweep():
    rng = np.random.default_rng(37)
    n = H * W * CH
    ws = np.zeros(1 << 16, np.uint8)
    val, sd = floats(rng, n, lo=-3.0, hi=5.0), stds_like(rng, n)
    for lo, hi in ((0.0, 1.0), (-3.0, 5.0)):
        for bins in (1, 2, 7, 64):
            edges = np.linspace(lo, hi, bins + 1)
            v = val.copy()
            v[3:3 + bins + 1] = edges                                     # every edge, and its two neighbours
            v[40:40 + bins + 1] = np.nextafter(edges, -np.inf)
            v[80:80 + bins + 1] = np.nextafter(edges, np.inf)
            for with_std in (False, True):
                for mask in (7, 5):
                    out = np.full((CH, bins), -7.0)
                    rc = L.hm_channel_histogram(p(v), p(sd) if with_std else None, n, CH, mask, p(edges), bins, lo, hi, p(out), p(ws), None)
                    report(f"channel_histogram [{lo},{hi}] bins={bins} std={int(with_std)} mask={mask}", rc, hist=out)
    for with_std in (False, True):
        out = np.full((CH, 2), -7.0)
        report(f"channel_minmax std={int(with_std)}", L.hm_channel_minmax(p(val), p(sd) if with_std else None, n, CH, p(out), p(ws), None), mm=out)
    for nf in (2, 5):
        vals = [floats(rng, n, lo=0.0, hi=1.0) * 2.0 ** i for i in range(nf)]
        stds = [stds_like(rng, n) for _ in range(nf)]
        pi, pj = zip(*[(i, j) for i in range(nf) for j in range(i + 1, nf)][:nat.HM_PAIRS_MAX])
        npairs = len(pi)
        ci, cj = (C.c_int32 * npairs)(*pi), (C.c_int32 * npairs)(*pj)
        mult = d3(*[2.0 ** (i - j) for i, j in zip(pi, pj)])
        for with_std in (False, True):
            for thr in (False, True):
                lower, upper = (d3(0.05, 0.02, 0.0), d3(0.9, 1.5, 3.0)) if thr else (None, None)
                sp = ptrs(stds) if with_std else None
                mm = np.full((npairs, 2, CH, 2), -7.0)
                rc = L.hm_pairs_minmax(ptrs(vals), sp, nf, ci, cj, mult, npairs, n, CH, lower, upper, p(mm), p(ws), None)
                report(f"pairs_minmax N={nf} std={int(with_std)} thr={int(thr)}", rc, mm=mm)
                for bins in (1, 7, 32):
                    edges = np.empty((npairs, 2, CH, bins + 1))
                    for idx in np.ndindex(npairs, 2, CH):
                        lo, hi = mm[idx]
                        if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
                            lo, hi = -1.0, 1.0
                        edges[idx] = np.linspace(lo, hi, bins + 1)
                    out = np.full((npairs, 2, CH, bins), -7.0)
                    rc = L.hm_pairs_histogram(ptrs(vals), sp, nf, ci, cj, mult, npairs, n, CH, 7, lower, upper, p(edges), bins, p(out), p(ws), None)
                    report(f"pairs_histogram N={nf} std={int(with_std)} thr={int(thr)} bins={bins}", rc, hist=out)


# ---- producers ---------------------------------------------------------------------------------------------------------------------
def producer_sweep():
    rng = np.random.default_rng(53)
    n = H * W * CH
    mean = floats(rng, n, lo=-0.1, hi=1.1)
    mean[20:31] = (np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.5, 256.0, -1.0, 1e30, 3.49999, 127.5])) / 255.0
    m2 = np.abs(floats(rng, n, lo=0.0, hi=4000.0))
    for count in (2, 7):
        om, os_ = np.full(n, 9, np.uint8), np.full(n, 9, np.uint8)
        report(f"welford_finalize count={count}", L.hm_welford_finalize(p(mean), p(m2), count, p(om), p(os_), n, None), mean=om, std=os_)
    rng_w = np.random.default_rng(59)                                   # a generator of its own: the later cases keep their inputs
    for bits in (9, 12, 16):
        top = float((1 << bits) - 1)
        mean16 = mean * 255.0 / top                                      # the same multiples of 1 / 2 once scaled by 2^bits - 1
        mean16[20:31] = np.array([0.5, 1.5, 2.5, top - 0.5, top + 0.5, -0.5, top + 1.0, -1.0, 1e30, 3.49999, (top + 1.0) / 2.0 - 0.5]) / top
        for count in (2, 7):
            om, os_ = np.full(n, 9, np.uint16), np.full(n, 9, np.uint16)
            rc = L.hm_welford_finalize_u16(p(mean16), p(m2), count, bits, p(om), p(os_), n, None)
            report(f"welford_finalize_u16 bits={bits} count={count}", rc, mean=om, std=os_)
    # the update entries: seeded frames, a NaN and an inf in the mean and in m2 when count_before > 0, with and without ICRF and m2
    nf = 5
    for count_before in (0, 3):
        state = rng_w.uniform(0.0, 1.0, size=n) if count_before else np.zeros(n)
        sq = rng_w.uniform(0.0, 0.5, size=n) if count_before else np.zeros(n)
        if count_before:
            state[7], state[8], sq[9], sq[10] = np.nan, np.inf, np.nan, np.inf
        for with_icrf in (False, True):
            for with_m2 in (False, True):
                frames = [rng_w.integers(0, 256, size=n, dtype=np.uint8) for _ in range(nf)]
                icrf, _ = tables(rng_w, 256, CH)
                m, q = state.copy(), (sq.copy() if with_m2 else None)
                rc = L.hm_welford_update(ptrs(frames), nf, count_before, p(icrf) if with_icrf else None, p(m), p(q), n, CH, None)
                report(f"welford_update count_before={count_before} icrf={int(with_icrf)} m2={int(with_m2)}", rc, mean=m, m2=q)
                for bits in (9, 12, 16):
                    frames16 = [rng_w.integers(0, 1 << bits, size=n, dtype=np.uint16) for _ in range(nf)]
                    if bits < 16:
                        frames16[1][::5] |= np.uint16(1 << bits)                # stray high bits: masked away
                        frames16[3][::3] |= np.uint16(0x8000)
                    icrf16, _ = tables(rng_w, 1 << bits, CH)
                    m, q = state.copy(), (sq.copy() if with_m2 else None)
                    rc = L.hm_welford_update_u16(ptrs(frames16), nf, count_before, p(icrf16) if with_icrf else None, p(m), p(q), n, CH, bits, 0, None)
                    report(f"welford_update_u16 bits={bits} count_before={count_before} icrf={int(with_icrf)} m2={int(with_m2)}", rc, mean=m, m2=q)
    for ch in (1, 3):
        for fill in ("bell", "sparse", "flat"):
            prof = np.zeros((256, 256, ch), np.int64)
            i = np.arange(256)[:, None, None]
            f = np.arange(256)[None, :, None]
            if fill == "bell":
                prof += (1000.0 * np.exp(-0.5 * ((f - i) / (2.0 + i / 64.0)) ** 2)).astype(np.int64) + rng.integers(0, 3, size=prof.shape)
            elif fill == "sparse":
                prof += rng.integers(0, 50, size=prof.shape) * (rng.uniform(size=prof.shape) < 0.3)
            else:
                prof += rng.integers(0, 4, size=prof.shape)
            report(f"noise_profile_clean_edges C={ch} {fill}", L.hm_noise_profile_clean_edges(p(prof), ch, None), prof=prof)
    val, sd = floats(rng, n, lo=-1.0, hi=2.0), stds_like(rng, n)
    grid = np.linspace(-1.5, 2.5, 33)
    for with_std in (False, True):
        for ch in range(CH):
            mom = np.full(nat.HM_KDE_MOMENTS, -7.0)
            report(f"kde_moments std={int(with_std)} channel={ch}", L.hm_kde_moments(p(val), p(sd) if with_std else None, n, CH, ch, p(mom), None, 0, None),
                   moments=mom)
            out = np.full(grid.size, -7.0)
            rc = L.hm_kde_evaluate(p(val), p(sd) if with_std else None, n, CH, ch, 0.21, 0.37, p(grid), grid.size, p(out), None, 0, None)
            report(f"kde_evaluate std={int(with_std)} channel={ch}", rc, density=out)
    # differential evolution: three generations of one problem from a zeroed status
    S, P, N, npx = 8, 3, 3, H * W
    dn = np.sort(rng.integers(0, 256, size=(npx, N), dtype=np.uint8), axis=1)
    mean_icrf = np.linspace(0.0, 1.0, 256) ** 1.3
    pca = 0.02 * np.stack([np.sin(np.pi * (k + 1) * np.linspace(0.0, 1.0, 256)) for k in range(P)], axis=1).copy()
    lo_l, hi_l = np.full(P, -1.0), np.full(P, 1.0)
    for with_std in (False, True):
        sd_px = stds_like(rng, (npx, N), zeros=False) if with_std else None
        pop = rng.uniform(size=(S, P))
        en, trial, ten = np.full(S, np.inf), np.zeros((S, P)), np.zeros(S)
        icrf, valid, status = np.zeros((S, 256)), np.zeros(S, np.uint8), np.zeros(nat.HM_DE_STATUS_WORDS, np.int64)
        for g in range(3):
            rc = L.hm_de_generation(p(pop), p(en), p(trial), p(ten), p(icrf), p(valid), p(status), p(mean_icrf), p(pca), p(lo_l), p(hi_l), p(dn),
                                    p(sd_px), d3(0.01, 0.02, 0.04), npx, N, 5, 250, S, P, 1234, 50, 0.5, 1.0, 0.7, 0.01, -1.0, None, None)
            report(f"de_generation std={int(with_std)} g={g}", rc, pop=pop, energies=en, trial=trial, trial_energies=ten, icrf=icrf, valid=valid,
                   status=status)


if __name__ == "__main__":
    merge_sweep()
    frame_sweep()
    ops_sweep()
    stats_sweep()
    producer_sweep()
