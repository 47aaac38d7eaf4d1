"""The mean / std reductions at the limits of their ABI: hm_channel_statistics (csrc/hm_stats.hip: k_stats, k_stats_final),
hm_pair_statistics (k_pair_stats, k_pair_final), hm_pairs_statistics (k_pairs_stats, k_pairs_stats_lds<STD, NI, THR>, k_pairs_final;
csrc/hm_pointwise.hip: k_thresholds), hm_axis_statistics (csrc/hm_stats_axis.hip: k_axis_thread, k_axis_row, k_axis_final,
k_axis_final_tree) and hm_axis_statistics2 (k_axis_final2, k_axis_final2_tree), on the HOST build (csrc_host/hm_host.cpp), against a np.longdouble reference written here. The checks are functions
of a device name: tests/test_gpu_moment_limits.py runs the same ones on the MI355X (and alone runs the sizes whose path - the mid-stream
block fold - only the device build has).

Reference (line_reference), per output line (one channel, one output element, or one pair, kind and channel), as
modules/measurand.py:339-349 count: W = nansum(w) (a NaN value with a finite std still counts), m = nansum(w v) / W,
Q = nansum(w (v - m)^2), sigma = sqrt(Q / W), error = nanmean(std). Channel / axis statistics: w = float64(1 / std) is one IEEE division in
every implementation and is formed in float64, then promoted. Pair kernels: scale = mult y and a = x - scale stay float64; r, the two
variances, w = 1 / sqrt(q) and s = sqrt(q) are formed in longdouble from the float64 inputs. R = max |v_i - m| over the counted elements
(channel / axis kernels: those with w != 0, which weighted_first() passes over; pair kernels: every one - acc_add_pair keeps a lane's first
element as its shift whatever its weight, the documented limit). test_reference_is_the_oracle pins it to oracle.dimension_statistics /
compute_difference at 1e-13.

Bound (moment_bounds), u = 2^-53. A state is (W, c, M) with M the moment about ITS OWN c; in exact arithmetic Chan's merges of such states
are exact, so what reaches the result is, once each: the rounding of a block's shifted sums (every |v - K| <= 2R: K is an element or a
running mean), of the means the folds and merges difference, and of the sums of weights.
    depth    chain  elements a lane adds between two folds: min(lane elements, 64 + 3)           (kMomBlock, + the 1-3 tail positions)
             L      folds of the lane (it == 0, every 64 elements, acc_finish) + merges above it   (see stream_depth / axis_depth)
             wall   elements of the lane (m.Wall += w runs over all of them, unblocked)
    mean     |got - m| <= (8 + 2 chain + 9 L + wall) u (|m| + 2R) + pert_m
             S1 / S0: (chain + 4) on 2R;  a fold or merge: d, f (rcp_nr: 3 u), d f, the sum: <= 7 u (|m| + 2R), and its W: u;  the
             finish (W mean) / Wall: the chains of W (chain + L) and Wall (wall + L) and 4 more
    std      |got - sigma| / sigma <= u [2 (chain + L) (2R / sigma)^2 + 7 L (|m| + 2R) 2R / sigma^2] + (5 L + wall / 2 + 6) u
                                      + (2 X e_m + W e_m^2 / 2) / Q + pert_s
             first term: S2 (chain + 3) and S1 q through the shift, 2 (chain + 2), on (2R)^2 W, halved for the root;  second: the 7 u
             (|m| + 2R) of each fold / merge displaces that state's centre, at a lever <= 2R;  third: the <= 10 u a merge's own products
             and sums put on M, Wall's chain, the division and the root;  fourth: the moment is taken about the COMPUTED mean, e_m = the
             bound on the mean away from m: first order only when W != Wall, X = |sum_counted w (v - m)|, and W e_m^2 in second order,
             which is what counts where |m| / sigma is large (the offset family)
    error    (wall + L + 2) u sum|s| / count + pert_e                                                (the ROI-mean bound)
    each is at least u (|m| + 2R) resp. u 2R, and where sigma = 0 the std's is e_m (sqrt(0 + e_m^2)), so lines with one or with identical
    counted elements need no separate allowance. (The device build's shifted sums give exactly 0 there, asserted apart.)
    Host build: two passes of running sums - chain = wall = the line's length, L = 0, and the first std term is (chain + 4) u (sum of
    positive terms: no (2R / sigma)^2).
    Pair kernels, per element (pert_*, first order in a relative perturbation eps_v of each value, eps_w of each weight, eps_s of each
    std: mean eps_v sum|w v| / W + 2 eps_w sum|w||v - m| / |W|; std eps_w + eps_v sum|w||v - m||v| / Q; error eps_s sum|s| / count),
    in u, with rcp at 1.00 ulp = 2 u and rsq at 1.25 ulp = 2.5 u - see PAIR_EPS.
Counts and the NaN pattern are exact. On every benign case the DEVICE bound (its geometry is host arithmetic, read from the HIP library
where an entry point gives it) on the mean, relative to |m| + 2R, and on the std, relative to sigma, is asserted <= 1e-11, the tolerance
of the older tests - on either build; the host build's own bound grows with the line's length and is not capped.

Heavy-tailed lines (an element of 1.4e6 with std 2.5e11 beside values of 0.05): the bound above with R over the w != 0 elements holds
and is printed, and is loose (R = 1.4e6). For the channel and axis kernels a second, sharper one is asserted: weighted_first() promises
that the shift is never the light element, so R is taken over the elements heavier than 1e-9 of the heaviest weight and the light ones
enter with their own w (|v - m| + 2R)^2 (tight=True). The pair kernels make no such promise and get the loose bound alone.

Stds that are all negative: the mean, the std and error = nanmean(std) < 0 of the reference under the same bound. Mixed signs are out of
scope: sum(1 / std) can cancel.

Every check records error / bound; the module prints the maxima per family and build."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from oracle import hdr_oracle as orc

from test_stats_limits_host import LD, U, T, backend, eng, family, is_cuda, offset_by_8

assert np.finfo(LD).nmant >= 63, "the references need an extended-precision np.longdouble (x87: 64-bit significand)"
WORST = {}                                                                  # family -> largest error / bound seen
CAP = 1e-11                                                                 # the older tests' tolerance: benign device bounds stay below


@pytest.fixture(scope="module", autouse=True)
def report_moment_maxima():
    """After the module's tests: the largest error of each family in units of its bound (DESIGN.md section 5 quotes them)."""
    yield
    print("\nobserved maxima, in units of the bound:", {k: float(f"{v:.3g}") for k, v in sorted(WORST.items())})


def record(fam, err, bound):
    err, bound = np.asarray(err, LD), np.asarray(bound, LD)
    with np.errstate(all="ignore"):
        ratio = np.where((err == 0) & (bound == 0), 0, err / bound)         # (one counted element: both are exactly 0)
    worst = float(ratio.max()) if err.size else 0.0
    WORST[fam] = max(WORST.get(fam, 0.0), worst)
    return worst


def to_np(t):
    return None if t is None else t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ reference
def line_reference(v, w=None, s=None, r_all=False, light=None):
    """v (lines, A) longdouble; w weights (longdouble, None = unweighted); s stds (for `error`). -> dict of (lines,) longdouble arrays.
    light: a fraction - R runs over the elements heavier than that fraction of the line's heaviest weight, the others enter `Slight`."""
    v = np.atleast_2d(np.asarray(v, LD))
    with np.errstate(all="ignore"):
        if w is None:
            cnt = ~np.isnan(v)
            wz = cnt.astype(LD)
            wall = wz.sum(1)
            vz = np.where(cnt, v, 0)
            t = vz
        else:
            w = np.atleast_2d(np.asarray(w, LD))
            wall = np.where(np.isnan(w), 0, w).sum(1)                       # nansum(weights)
            t = v * w
            cnt = ~np.isnan(t)                                              # nansum(values * weights)
            wz, vz, t = np.where(cnt, w, 0), np.where(cnt, v, 0), np.where(cnt, t, 0)
        m = t.sum(1) / wall
        d = vz - m[:, None]
        d = np.where(np.abs(d) <= 16 * np.finfo(LD).eps * np.abs(m)[:, None], 0, d)           # (the reference's own rounding of m: identical elements have d = 0)
        wd = wz * d
        q = wd * d
        Q = q.sum(1)
        sigma = np.sqrt(Q / wall)
        aw, ad = np.abs(wz), np.abs(d)
        sel = cnt if r_all else cnt & (wz != 0)
        out = dict(n=cnt.sum(1), W=wall, m=m, Q=Q, sigma=sigma, A1=np.abs(t).sum(1) / np.abs(wall), A2=(aw * ad).sum(1) / np.abs(wall),
                   B1=(aw * ad * np.abs(vz)).sum(1) / np.abs(Q), X=np.abs(wd.sum(1)), Slight=np.zeros(len(m), LD))
        if light is not None:
            heavy = sel & (aw > light * aw.max(1)[:, None])
            out["R"] = np.where(heavy, ad, 0).max(1)
            lt = sel & ~heavy
            out["Slight"] = np.where(lt, aw * (ad + 2 * out["R"][:, None]) ** 2, 0).sum(1)
            out["Wheavy"] = np.where(heavy, aw, 0).sum(1)
        else:
            out["R"] = np.where(sel, ad, 0).max(1)
        if s is not None:
            s = np.atleast_2d(np.asarray(s, LD))
            oks = ~np.isnan(s)
            out["cs"] = oks.sum(1)
            out["err"] = np.where(oks, s, 0).sum(1) / out["cs"]
            out["sabs"] = np.abs(np.where(oks, s, 0)).sum(1)
    return out


def weights_of(s):
    """float64 1 / std (one IEEE division everywhere), promoted."""
    with np.errstate(all="ignore"):
        return (1.0 / np.asarray(s, np.float64)).astype(LD)


def pair_lines(x, sx, y, sy, mult):
    """The two difference images of measurand.py:634-653 as reference lines: x, y (k, C) float64 -> [(v, w, s) for abs, rel], each (C, k)
    longdouble; w, s None without stds."""
    with np.errstate(all="ignore"):
        scale = mult * y                                                    # float64: one IEEE operation everywhere
        a = x - scale
        aL, scL, xL, yL, mL = a.astype(LD), scale.astype(LD), x.astype(LD), y.astype(LD), LD(mult)
        r = aL / scL
        if sx is None and sy is None:
            return [(aL.T, None, None), (r.T, None, None)]
        xs = np.zeros_like(xL) if sx is None else sx.astype(LD)
        ys = np.zeros_like(xL) if sy is None else sy.astype(LD)
        qa = xs * xs + (mL * ys) ** 2
        qr = (xs / (mL * yL)) ** 2 + ((ys * xL) / (mL * yL * yL)) ** 2
        return [(aL.T, (1 / np.sqrt(qa)).T, np.sqrt(qa).T), (r.T, (1 / np.sqrt(qr)).T, np.sqrt(qr).T)]


# per-element roundings of the pair kernels in u: (eps_v, eps_w, eps_s) for [abs, rel], with and without std.
#   hip   pair_terms(): inv = rcp_newton (2) ; r = a inv (+1) -> 3.  qa = xs xs + m1 m1, m1 = mult ys: <= 4; wa = rsq (2.5) + qa / 2 -> 4.5;
#         as = qa wa: qa / 2 + 2.5 + 1 -> 5.5.  u1 = xs inv: 3; u2 = ((ys xv) mult)(inv inv): 8; qr = u1 u1 + u2 u2: <= 18; wr: 9 + 2.5 -> 11.5;
#         rs = qr wr: 9 + 2.5 + 1 -> 12.5
#   host  diff_terms(): r = a / scale: 1.  qa: 4; as = sqrt: 2 + 1 -> 3; w = 1 / as: 4.  u1: 2, u2: 4, qr: <= 10; rs: 5 + 1 -> 6; w: 7
PAIR_EPS = {("hip", True): [(0, 4.5, 5.5), (3, 11.5, 12.5)], ("hip", False): [(0, 0, 0), (3, 0, 0)],
            ("host", True): [(0, 4, 3), (1, 7, 6)], ("host", False): [(0, 0, 0), (1, 0, 0)]}


# ------------------------------------------------------------------------------------------------ geometry -> depth
STAT_BLOCKS, MOM_BLOCK = 768, 64        # kStatBlocks, kMomBlock. stat_grid(): ceil(n / 256) workgroups of 256, rounded up to a multiple of 12, at most 768


def ceil_div(a, b):
    return -(-a // b)


def stat_grid(n, per=256):
    """stat_grid() of hm_moments.h: per = 256 in hm_channel_statistics and hm_pair_statistics, 64-lane workgroup rows (per = 64) in hm_pairs_statistics."""
    return min(STAT_BLOCKS, 12 * ceil_div(ceil_div(n, per), 12))


def lane_depth(n_lane, un, above):
    """A lane of n_lane elements that folds every 64 / un iterations of un elements, `above` merges over it."""
    folds = 2 + ceil_div(n_lane, un) // (MOM_BLOCK // un)                    # it == 0; (it & (64 / UN - 1)) == 64 / UN - 1; acc_finish
    return dict(chain=min(n_lane, MOM_BLOCK + 3), L=folds + above, wall=n_lane, folds=folds, twopass=False)


def host_depth(count):
    return dict(chain=count, L=0, wall=count, folds=0, twopass=True)        # line_statistics(): two passes of running sums


def stream_depth(hip, n, C_, un, per=256):
    """k_stats / k_pair_stats (per = 256: six shuffle steps and three LDS additions in block_merge_store, then grid_merge: ceil(grid / 256)
    serial merges and eight LDS steps) and the all-pairs kernels (per = 64: a wave per workgroup row, six shuffle steps, k_pairs_final)."""
    if not hip:
        return host_depth(n // C_)
    grid = stat_grid(n, per)
    return lane_depth(ceil_div(n, grid * per), un, 6 + (3 if per == 256 else 0) + ceil_div(grid, 256) + 8)


def axis_geometry(outer, A, inner):
    """(row, KS, tree) of axis_plan() / hm_axis_statistics: KS read back from the HIP library's workspace size (0 bytes = 1)."""
    ws = int(nat.hip_lib.hm_axis_statistics_workspace_bytes(outer, A, inner))
    assert ws % (48 * outer * inner) == 0
    KS = max(1, ws // (48 * outer * inner))
    return inner < 16 and A > 32, KS, KS >= 32 and outer * inner <= 4096


def stage1_lane(row, KS, A, inner):
    """-> (elements of a lane, merges inside the workgroup) of k_axis_thread / k_axis_row."""
    if not row:
        return ceil_div(A, KS), 0                                           # positions seg, seg + KS, ...
    Tm = (256 // inner) * inner
    return ceil_div(ceil_div(A, KS) * inner, Tm), math.ceil(math.log2(Tm // inner)) if Tm > inner else 0      # the halving tree over Tm / inner partials


def axis_depth(hip, outer, A, inner):
    if not hip:
        return host_depth(A)
    row, KS, tree = axis_geometry(outer, A, inner)
    n_lane, wg = stage1_lane(row, KS, A, inner)
    final = 0 if KS == 1 else (ceil_div(KS, 256) + 8 if tree else KS)       # k_axis_final_tree | k_axis_final
    return lane_depth(n_lane, 4, wg + final)


def axis2_geometry(outer, a1, mid, a2, inner):
    """Stage 1 of axis2_plan(): (outer1, A, inner1, R, row, KS, tree); KS from hm_axis_statistics2_workspace_bytes / (48 n_out1)."""
    o1, A, i1, R = (outer, a1, mid * a2 * inner, a2) if a1 >= a2 else (outer * a1 * mid, a2, inner, a1)
    ws = int(nat.hip_lib.hm_axis_statistics2_workspace_bytes(outer, a1, mid, a2, inner))
    assert ws % (48 * o1 * i1) == 0 and ws > 0
    KS = ws // (48 * o1 * i1)
    return o1, A, i1, R, i1 < 16 and A > 32, KS, R * KS >= 64 and outer * mid * inner <= 4096


def axis2_depth(hip, outer, a1, mid, a2, inner):
    if not hip:
        return host_depth(a1 * a2)
    o1, A, i1, R, row, KS, tree = axis2_geometry(outer, a1, mid, a2, inner)
    n_lane, wg = stage1_lane(row, KS, A, i1)
    return lane_depth(n_lane, 4, wg + (ceil_div(R * KS, 256) + 8 if tree else R * KS))        # k_axis_final2_tree | k_axis_final2


# ------------------------------------------------------------------------------------------------ bound
def moment_bounds(ref, depth, eps=(0, 0, 0), tight=False):
    """-> (mean bound, std bound, error bound or None, relative mean bound, relative std bound); longdouble arrays per line."""
    u = LD(U)
    chain, L, wall = depth["chain"], depth["L"], depth["wall"]
    m, R, sg, Q, W = np.abs(ref["m"]), ref["R"], ref["sigma"], np.abs(ref["Q"]), np.abs(ref["W"])
    ev, ew, es = (LD(e) for e in eps)
    with np.errstate(all="ignore"):
        scale = m + 2 * R
        mean_rel = (8 + 2 * chain + 9 * L + wall) * u
        e_m = np.maximum(mean_rel * scale + u * (ev * ref["A1"] + 2 * ew * ref["A2"]), u * scale)
        spread = (2 * R) ** 2 * (ref["Wheavy"] if tight else W) + ref["Slight"]               # sum w (v - K)^2 at its largest
        first = (chain + 4) * u if depth["twopass"] else 2 * (chain + L) * u * spread / Q
        rel = (first + 7 * L * u * scale * 2 * R * W / Q + (5 * L + wall / 2 + 6) * u + (2 * ref["X"] * e_m + W * e_m * e_m / 2) / Q
               + u * (ew + ev * ref["B1"]))
        rel = np.where(Q > 0, rel, 0)
        e_s = np.where(Q > 0, np.where(rel <= 0.1, sg * rel * (1 + rel), 2 * sg * rel), e_m)    # |sqrt(s^2 (1 + 2 rel)) - s|; sigma = 0: sqrt(e_m^2)
        e_s = np.maximum(e_s, u * 2 * R)
        e_e = None
        if "err" in ref:
            e_e = ((wall + L + 2) * u + es * u) * ref["sabs"] / ref["cs"]
        rel_m = np.where(scale > 0, e_m / scale, 0)
    return e_m, e_s, e_e, rel_m, rel


def assert_lines(device, fam, what, got, ref, depth, eps=(0, 0, 0), tight=False, cap_depth=None, eps_cap=None):
    """got = (mean, std, error or None) arrays per line. Lines with nothing counted and no weight: NaN where the reference's 0 / 0 is; all-NaN values
    under finite stds: the reference's 0 / W = 0 for the mean and the std, exactly."""
    fam = family(device, fam)
    gm, gs = np.asarray(got[0], np.float64).ravel(), np.asarray(got[1], np.float64).ravel()
    assert gm.shape == ref["m"].shape and gs.shape == ref["m"].shape, (what, gm.shape, ref["m"].shape)
    with np.errstate(all="ignore"):
        live = (ref["n"] > 0) | ((ref["W"] != 0) & np.isfinite(ref["W"]))       # nothing counted but weights: 0 / W = 0 and sqrt(0 / W) = 0, held to the bound (0)
    for k in ("W", "m", "Q", "sigma", "R"):
        assert np.all(np.isfinite(ref[k][live])), f"{what}: the reference's {k} is not finite - a case for the special-value checks"
    for g, r, name in ((gm, ref["m"], "mean"), (gs, ref["sigma"], "std")):
        assert np.array_equal(np.isnan(g), np.isnan(r)) and not np.isinf(g).any(), f"{what}: NaN / inf pattern of the {name}: {g[:8]} {r[:8]}"
    e_m, e_s, e_e, rel_m, rel_s = moment_bounds(ref, depth, eps, tight)
    if cap_depth is not None:                                               # benign: the DEVICE bound stays below the older tests' tolerance
        _, _, _, cm, cs = moment_bounds(ref, cap_depth, eps if eps_cap is None else eps_cap)
        assert float(cm[live].max()) <= CAP and float(cs[live].max()) <= CAP, f"{what}: derived device bound {float(cm[live].max()):.2e} / {float(cs[live].max()):.2e} above {CAP}"
    wm = record(fam + " mean", np.abs(gm[live].astype(LD) - ref["m"][live]), e_m[live])
    ws = record(fam + " std", np.abs(gs[live].astype(LD) - ref["sigma"][live]), e_s[live])
    print(f"\n{what} [{fam}]: mean {wm:.3f}, std {ws:.3f} x bound; relative bounds mean {float(rel_m[live].max()):.2e}, std {float(rel_s[live].max()):.2e}", end="")
    assert wm <= 1.0, f"{what}: mean at {wm:.3f} x its bound"
    assert ws <= 1.0, f"{what}: std at {ws:.3f} x its bound (relative bound {float(rel_s[live].max()):.2e})"
    if "err" in ref and got[2] is not None:
        ge = np.asarray(got[2], np.float64).ravel()
        assert np.array_equal(np.isnan(ge), np.isnan(ref["err"])), f"{what}: NaN pattern of the error"
        ok = ref["cs"] > 0
        if ok.any():
            we = record(fam + " error", np.abs(ge[ok].astype(LD) - ref["err"][ok]), np.maximum(e_e[ok], LD(U) * np.abs(ref["err"][ok])))
            assert we <= 1.0, f"{what}: error at {we:.3f} x its bound"
    elif got[2] is not None:
        assert np.all(np.isnan(np.asarray(got[2]))), f"{what}: error without std must be NaN"


# ------------------------------------------------------------------------------------------------ data
def benign(rng, shape, weighted=True, axis=None):
    """Roughly centred values (|m| <~ R; clipped at three sigma, which keeps (2R / sigma)^2 of the bound near 40), stds on [0.05, 0.15),
    5 % NaN values and 3 % NaN stds set independently: W != Wall in most lines."""
    v = np.clip(rng.standard_normal(shape), -3, 3) * 0.3 + 0.1
    if axis is not None and shape[axis] <= 8:         # short lines: a spread pattern + noise, so that none is ill-conditioned by chance (two survivors 1e-6 apart)
        A = shape[axis]
        pattern = rng.permuted(np.broadcast_to(np.linspace(-1, 1, A).reshape([-1 if d == axis else 1 for d in range(len(shape))]), shape).copy(), axis=axis)
        v = 0.1 + 0.3 * (pattern + 0.1 * np.clip(rng.standard_normal(shape), -3, 3) / max(A - 1, 1))
    v[rng.random(shape) < 0.05] = np.nan
    if not weighted:
        return v, None
    s = 0.05 + 0.1 * rng.random(shape)
    s[rng.random(shape) < 0.03] = np.nan
    return v, s


def offset_data(rng, shape, weighted=True):
    """Mean 1e6, spread 1e-3 (the data of test_one_pass_statistics_are_stable): the |m| term of the bound."""
    v = 1e6 + 1e-3 * rng.standard_normal(shape)
    return v, (0.05 + 0.1 * rng.random(shape) if weighted else None)


def heavy_tailed(rng, shape):
    """Values near 0.05 with stds near 0.0185; the callers plant the element 1.4e6 with std 2.5e11 (weight 4e-12)."""
    return 0.05 + 0.01 * rng.standard_normal(shape), 0.0185 * (1 + 0.05 * rng.random(shape))


HEAVY_V, HEAVY_S, LIGHT = 1.4e6, 2.5e11, 1e-9


def pair_frames(rng, k, C_, with_std=True, nan=0.10):
    """x, y on [0.5, 1.2) with 10 % NaNs placed jointly in value and std. (Narrowed from [0.2, 1.2): there x / y spans 0.17 .. 6 and the weighted
    relative difference's (|m| + 2R) 2R / sigma^2 takes the derived device bound to 1.2e-11, above the cap.)"""
    out = []
    for _ in range(2):
        v = 0.5 + 0.7 * rng.random((k, C_))
        s = 0.01 + 0.02 * rng.random((k, C_))
        hole = rng.random((k, C_)) < nan
        v[hole] = np.nan
        s[hole] = np.nan
        out += [v, s if with_std else None]
    return out                                                              # x, sx, y, sy


# ------------------------------------------------------------------------------------------------ hm_channel_statistics
def run_channel(device, v, s, off8=False):
    mk = offset_by_8 if off8 else T
    got = eng(device, "channel_statistics", mk(v, device), None if s is None else mk(s, device))
    return to_np(got["mean"]), to_np(got["std"]), to_np(got["error"])


def channel_reference(v, s, light=None):
    refs = [line_reference(v[:, c].astype(LD), None if s is None else weights_of(s[:, c]), None if s is None else s[:, c].astype(LD), light=light)
            for c in range(v.shape[1])]                                     # (a channel at a time: the two-fold sizes are 8 M elements each)
    return {k: np.concatenate([r[k] for r in refs]) for k in refs[0]}


def check_channel(device, n, C_, weighted, fam="benign", off8=False, seed=0):
    """n elements of C_ channels; UN = 4 chunks of 64 per wave iteration weighted, 8 unweighted (HM_STATS_UN_NOSTD)."""
    assert n % C_ == 0
    rng = np.random.default_rng(1000 * C_ + n % 9973 + seed)
    v, s = (benign if fam == "benign" else offset_data)(rng, (n // C_, C_), weighted)
    got = run_channel(device, v, s, off8)
    un = 4 if weighted else 8
    cap = stream_depth(True, n, C_, un) if fam == "benign" else None
    assert_lines(device, f"channel {fam}", f"channel n={n} C={C_} weighted={weighted}", got, channel_reference(v, s),
                 stream_depth(is_cuda(device), n, C_, un), cap_depth=cap)


CHANNEL_SMALL = [200, 196608, 196608 - 1, 196608 + 1]                        # x C / C: tail only; 768 x 256, the grid exactly full, -+ a pixel
TWO_FOLDS = 2 * 12582912                                                    # 64 iterations of 4 x 196 608 weighted elements, twice


def channel_sizes(C_, weighted):
    un = 4 if weighted else 8
    first = 768 * 256 * un                                                   # the first whole-chunk iteration of every wave
    return [(200 // C_) * C_, (196608 // C_) * C_ - C_, (196608 // C_) * C_, (196608 // C_) * C_ + C_, ceil_div(first, C_) * C_ + 37 * C_]


def check_channel_heavy(device, C_=3):
    """The weighted_first() case at a lane's first element (index 0) and at the first element of its second block (its fifth: index
    4 x 196 608 - after the early fold the shift is the running mean); both of channel 0."""
    n = 5 * 196608 + 37 * C_
    rng = np.random.default_rng(5)
    v, s = heavy_tailed(rng, (n // C_, C_))
    for e in (0, 4 * 196608):
        assert e % C_ == 0
        v[e // C_, 0], s[e // C_, 0] = HEAVY_V, HEAVY_S
    got = run_channel(device, v, s)
    depth = stream_depth(is_cuda(device), n, C_, 4)
    assert_lines(device, "channel heavy-tailed (loose)", "channel heavy-tailed, R over w != 0", got, channel_reference(v, s), depth)
    assert_lines(device, "channel heavy-tailed", "channel heavy-tailed, R over the heavy elements", got, channel_reference(v, s, LIGHT), depth, tight=True)


def check_channel_negative(device, C_=3, n=3 * 4099):
    """Every std negative: w < 0 throughout, sum w (v - m)^2 and sum w both negative, the std the ordinary positive one."""
    rng = np.random.default_rng(6)
    v, s = benign(rng, (n // C_, C_))
    got = run_channel(device, v, -s)
    ref = channel_reference(v, -s)
    assert np.all(ref["err"] < 0) and np.all(ref["sigma"] > 0.1) and np.all(ref["W"] < 0)
    assert_lines(device, "negative stds", "channel, all stds negative", got, ref, stream_depth(is_cuda(device), n, C_, 4))
    x = v.reshape(1, -1, C_)
    got = raw_axis(device, x, -s.reshape(x.shape))
    assert_lines(device, "negative stds", "axis (row kernel), all stds negative", got, axis_reference(x, -s.reshape(x.shape)), axis_depth(is_cuda(device), *x.shape))


# ------------------------------------------------------------------------------------------------ hm_axis_statistics / hm_axis_statistics2
def raw_axis(device, x, s, with_err=True, off8=False, expect=nat.HM_OK):
    """hm_axis_statistics through the C ABI on the dense (outer, A, inner) array x -> (mean, std, error or None), outputs pre-filled with 7."""
    outer, A, inner = x.shape
    mk = offset_by_8 if off8 else T
    with backend(device) as (lib, stream):
        xv = mk(x, device)
        sv = None if s is None else mk(s, device)
        o = [torch.full((outer * inner,), 7.0, dtype=torch.float64, device=device) for _ in range(3)]
        ws = torch.empty(max(1, int(lib.hm_axis_statistics_workspace_bytes(outer, A, inner)) // 8), dtype=torch.float64, device=device)
        rc = lib.hm_axis_statistics(xv.data_ptr(), nat.ptr(sv), outer, A, inner, o[0].data_ptr(), o[1].data_ptr(),
                                    o[2].data_ptr() if with_err else None, ws.data_ptr(), stream)
        assert rc == expect, (rc, expect)
        if not with_err:
            assert np.all(to_np(o[2]) == 7.0)
        return to_np(o[0]), to_np(o[1]), to_np(o[2]) if with_err and s is not None else None


def raw_axis2(device, x, s):
    outer, a1, mid, a2, inner = x.shape
    with backend(device) as (lib, stream):
        xv = T(x, device)
        sv = None if s is None else T(s, device)
        o = [torch.full((outer * mid * inner,), 7.0, dtype=torch.float64, device=device) for _ in range(3)]
        ws = torch.empty(max(1, int(lib.hm_axis_statistics2_workspace_bytes(*x.shape)) // 8), dtype=torch.float64, device=device)
        rc = lib.hm_axis_statistics2(xv.data_ptr(), nat.ptr(sv), *x.shape, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), ws.data_ptr(), stream)
        assert rc == nat.HM_OK, rc
        return to_np(o[0]), to_np(o[1]), to_np(o[2]) if s is not None else None


def axis_reference(x, s, light=None):
    lines = lambda a: np.moveaxis(a, 1, -1).reshape(-1, a.shape[1])         # noqa: E731  (outer * inner, A)
    return line_reference(lines(x).astype(LD), None if s is None else weights_of(lines(s)), None if s is None else lines(s).astype(LD), light=light)


def axis2_reference(x, s):
    outer, a1, mid, a2, inner = x.shape
    lines = lambda a: a.transpose(0, 2, 4, 1, 3).reshape(outer * mid * inner, a1 * a2)      # noqa: E731
    return line_reference(lines(x).astype(LD), None if s is None else weights_of(lines(s)), None if s is None else lines(s).astype(LD))


# (outer, A, inner) -> (row kernel, KS, tree final) as axis_plan() and hm_axis_statistics decide; every case asserts what it was built for
AXIS_THREAD = {(1, a, i): (False, 1, False) for a in (1, 2, 3, 4, 5, 7) for i in (16, 300)}
AXIS_THREAD.update({
    (1, 320, 16): (False, 20, False),          # KS capped by A / 16; serial k_axis_final
    (1, 33280, 16): (False, 256, True),        # KS = 256: 130-element segments - two folds and a tail; k_axis_final_tree
    (1, 64, 5000): (False, 4, False),          # n_out > 4096 with KS > 1: serial final
    (1, 16 * 20 + 1, 16): (False, 20, False),  # KS does not divide A
    (2, 5, 131072): (False, 1, False),         # 1024 workgroups: KS = 1
    (3, 200, 40): (False, 12, False),          # short inner >= 16: one workgroup, KS capped at 200 / 16
    (5, 32, 1): (False, 2, False), (5, 32, 3): (False, 2, False), (5, 7, 15): (False, 1, False), (2000, 3, 3): (False, 1, False),  # A <= 32, inner < 16: the channel-axis case
})
AXIS_ROW = {(o, 33, i): (True, 1, False) for o in (1, 1024) for i in (1, 3, 7, 15)}
AXIS_ROW.update({
    (70000, 33, 1): (True, 1, False), (70000, 33, 3): (True, 1, False),      # gridDim.y capped at 65 535: the o loop runs twice
    (1, 5000, 1): (True, 2, False), (1, 30000, 3): (True, 44, True), (1, 9000, 7): (True, 31, False), (1, 6000, 15): (True, 44, True),   # KS > 1
    (1, 139265, 15): (True, 1024, True),       # KS = 1024, seg_k = 137: the last segments start past the end
})


# Device only (16 M - 35 M elements each: seconds of longdouble reference per case, and nothing the host build does differently): KS = 1 and a
# chain of 130 per thread, the smallest with outer >= 1024; the capped gridDim.y with Tm = 252 (inner = 7: four idle threads store empty
# states into `red` on the second pass of the o loop) and Tm = 255 (inner = 15)
AXIS_ROW_LONG = {(1024, 130 * 85, 3): (True, 1, False), (70000, 33, 7): (True, 1, False), (70000, 33, 15): (True, 1, False)}


def check_axis(device, shape, weighted, expect, fam="benign", with_err=True, off8=False):
    outer, A, inner = shape
    assert axis_geometry(*shape) == expect, (shape, axis_geometry(*shape), expect)
    rng = np.random.default_rng(outer + 31 * A + 977 * inner)
    x, s = benign(rng, shape, weighted, axis=1) if fam == "benign" else offset_data(rng, shape, weighted)
    if fam == "benign" and A > 8 and outer * inner > 1:
        x[0, :, 0] = np.nan                                                 # an all-NaN line beside full ones
    got = raw_axis(device, x, s, with_err, off8)
    assert_lines(device, f"axis {fam}", f"axis {shape} weighted={weighted}", got, axis_reference(x, s), axis_depth(is_cuda(device), *shape),
                 cap_depth=axis_depth(True, *shape) if fam == "benign" else None)


def with_err_for(shape):
    """out_err NULL on a third of the shapes of either kernel, odd and even A among them."""
    return sum(shape) % 3 != 0


def check_axis_empty_segments(device):
    """(1, 139 265, 15): KS = 1024 segments of 137 positions cover 140 288 > A: the last ones are empty."""
    row, KS, _ = axis_geometry(1, 139265, 15)
    assert row and KS == 1024 and (KS - 1) * ceil_div(139265, KS) >= 139265


def check_axis_heavy(device):
    """Thread kernel (1, 200, 16), KS = 12: the outlier at segment 0's first position (k = 0) and at the first position of a lane's second
    block (its fifth: k = 4 KS). Row kernel: (1024, 33, 3), KS = 1: thread 0's first element; (1, 6000, 15), Tm = 255 = 17 positions: thread 0's
    first and fifth element."""
    for shape, spots in (((1, 200, 16), [(0, 0, 0), (0, 48, 0), (0, 1, 5)]), ((1024, 33, 3), [(0, 0, 0), (7, 0, 1)]),
                         ((1, 6000, 15), [(0, 0, 0), (0, 4 * 17, 0)])):
        rng = np.random.default_rng(shape[1])
        x, s = heavy_tailed(rng, shape)
        for sp in spots:
            x[sp], s[sp] = HEAVY_V, HEAVY_S
        got = raw_axis(device, x, s)
        depth = axis_depth(is_cuda(device), *shape)
        assert_lines(device, "axis heavy-tailed (loose)", f"axis heavy-tailed {shape}", got, axis_reference(x, s), depth)
        if shape[1] * shape[2] < 2 * 255:
            # a row of 99 elements on Tm = 255 threads: no thread holds two, so weighted_first() never sees a second element - the light one
            # is a state of its own and mom_merge() differences its mean 1.4e6 against 0.05. The sharper bound's premise (a lane that holds
            # a light element also holds a heavy one) does not apply; measured on the MI355X: mean 2.6e-11 of |m| + 2R, std 2.4e-10 relative
            # (DESIGN.md section 8, item 7).
            continue
        assert_lines(device, "axis heavy-tailed", f"axis heavy-tailed {shape}, R over the heavy elements", got, axis_reference(x, s, LIGHT), depth, tight=True)


# (outer, a1, mid, a2, inner) -> (stage 1 over a1, row kernel, KS, tree final)
AXIS2 = {
    (2, 11, 3, 5, 7): (True, False, 1, False),        # stage 1 over a1 (thread kernel, inner' = 105); R KS = 5: serial
    (2, 5, 3, 11, 7): (False, False, 1, False),       # stage 1 over a2 (outer' = 30, thread kernel: A <= 32)
    (3, 7, 2, 7, 5): (True, False, 1, False),         # a1 == a2
    (1, 63, 1, 1, 1): (True, True, 1, False),         # mid = inner = 1 (and a2 = 1): the merged axis
    (1, 9, 2, 7, 16): (True, False, 1, False), (1, 9, 2, 8, 16): (True, False, 1, False),
    (1, 160, 1, 3, 16): (True, False, 10, False), (1, 352, 1, 3, 16): (True, False, 22, True),          # thread kernel, KS > 1: R KS = 30 serial, 66 tree
    (1, 63, 1, 64, 1): (False, True, 1, False),       # stage 1 over a2 is the row kernel (outer' = 63, inner' = 1); R KS = 63: serial
    (1, 64, 1, 65, 1): (False, True, 1, True),        # ... R KS = 64: tree
    (1, 512, 4096, 2, 1): (True, False, 32, True), (1, 512, 4097, 2, 1): (True, False, 32, False),      # R KS = 64 with n_out2 at 4096 (tree) and 4097 (serial)
    (2, 3, 1, 5, 1): (False, False, 1, False), (1, 3, 5, 7, 1): (False, False, 1, False), (1, 5, 1, 3, 11): (True, False, 1, False),   # outer, mid, inner alone > 1
}


def check_axis2(device, shape, weighted, expect):
    outer, a1, mid, a2, inner = shape
    o1, A, i1, R, row, KS, tree = axis2_geometry(*shape)
    assert (a1 >= a2, row, KS, tree) == expect, (shape, (a1 >= a2, row, KS, tree), expect)
    rng = np.random.default_rng(sum(p * d for p, d in zip((3, 5, 7, 11, 13), shape)))
    x, s = benign(rng, shape, weighted)
    got = raw_axis2(device, x, s)
    ref = axis2_reference(x, s)
    assert_lines(device, "axis2 benign", f"axis2 {shape} weighted={weighted}", got, ref, axis2_depth(is_cuda(device), *shape),
                 cap_depth=axis2_depth(True, *shape))
    if mid == 1 and inner == 1 and a2 == 1:                                 # the merged axis: hm_axis_statistics on (outer, a1 a2, 1) under its own bound
        x1, s1 = x.reshape(outer, a1, 1), None if s is None else s.reshape(outer, a1, 1)
        assert_lines(device, "axis benign", f"axis {x1.shape} as axis2", raw_axis(device, x1, s1), ref, axis_depth(is_cuda(device), *x1.shape))


# ------------------------------------------------------------------------------------------------ pair kernels
def stats6(ab, rel):
    return [[to_np(d["mean"]), to_np(d["std"]), to_np(d["error"])] for d in (ab, rel)]


def assert_pair(device, fam, what, got6, x, sx, y, sy, mult, depth, cap_depth=None, r_all=True):
    """got6 = [[mean, std, error] of abs, of rel]; each kind's C lines against the reference under the kind's per-element roundings."""
    build, std = "hip" if is_cuda(device) else "host", sx is not None or sy is not None
    for h, (v, w, s) in enumerate(pair_lines(x, sx, y, sy, mult)):
        ref = line_reference(v, w, s, r_all=r_all)
        assert_lines(device, fam, f"{what} {'abs' if h == 0 else 'rel'}", got6[h], ref, depth, PAIR_EPS[(build, std)][h],
                     cap_depth=cap_depth, eps_cap=PAIR_EPS[("hip", std)][h])


def run_pair(device, x, sx, y, sy, mult, off8=False):
    mk = offset_by_8 if off8 else T
    up = lambda a: None if a is None else mk(a, device)                     # noqa: E731
    return stats6(*eng(device, "pair_statistics", up(x), up(sx), up(y), up(sy), mult))


def pair_un(sx, sy):
    return 2 if (sx is not None or sy is not None) else 4                   # kPairUN | HM_PAIR_UN_NOSTD


def check_pair(device, n, C_, SX, SY, mult, seed=0, off8=False):
    assert n % C_ == 0
    rng = np.random.default_rng(7000 + 13 * C_ + n % 9973 + seed)
    x, sx, y, sy = pair_frames(rng, n // C_, C_)
    sx, sy = (sx if SX else None), (sy if SY else None)
    got = run_pair(device, x, sx, y, sy, mult, off8)
    un = pair_un(sx, sy)
    assert_pair(device, "pair benign", f"pair n={n} C={C_} <{SX},{SY}> m={mult}", got, x, sx, y, sy, mult, stream_depth(is_cuda(device), n, C_, un),
                cap_depth=stream_depth(True, n, C_, un))


def pair_sizes(C_, std):
    first = 768 * 256 * (2 if std else 4)
    return [(200 // C_) * C_, (196608 // C_) * C_ - C_, (196608 // C_) * C_, (196608 // C_) * C_ + C_, ceil_div(first, C_) * C_ + 37 * C_]


def check_pair_heavy(device, C_=3):
    """y near 0 in one element: a relative difference of 1.4e6-class with a huge std - at a lane's first element and at the first of its
    second block. acc_add_pair keeps that element as the lane's shift: the bound carries R over ALL elements and is loose by construction."""
    n = 5 * 196608 + 37 * C_
    rng = np.random.default_rng(8)
    x, sx, y, sy = pair_frames(rng, n // C_, C_, nan=0.0)
    for e in (0, 2 * 196608):
        y[e // C_, 0], x[e // C_, 0] = 5e-7, 0.7
    got = run_pair(device, x, sx, y, sy, 1.0)
    assert_pair(device, "pair heavy-tailed (loose)", "pair heavy-tailed", got, x, sx, y, sy, 1.0, stream_depth(is_cuda(device), n, C_, 2))


def check_pair_one_special_lane(device, C_=3):
    """One frame where the `special` ballot of pair_process fires in exactly one lane of one wave: a single y = 0 (scale = 0 -> 1 / scale = inf, the relative difference infinite):
    the wave redoes its element with the guarded terms, every other wave keeps the fast path; the oracle's pattern and finite numbers."""
    n = 196608 + 37 * C_
    rng = np.random.default_rng(9)
    x, sx, y, sy = pair_frames(rng, n // C_, C_, nan=0.0)
    y[1000, 1] = 0.0                                                        # scale = 0: rel = +-inf, 1 / scale = inf
    check_pair_special(device, x, sx, y, sy, 0.5, "one special lane")
    check_pair_special(device, x, None, y, None, 0.5, "one special lane, no std")


def oracle_pair(x, sx, y, sy, mult):
    with np.errstate(all="ignore"):
        ad, ads, rd, rds = orc.compute_difference(x, sx, y, sy, mult)
        return [orc.dimension_statistics(ad, ads, 0), orc.dimension_statistics(rd, rds, 0)]


def assert_like_oracle(what, got, ref, rtol=1e-11):
    """NaN, +inf, -inf element for element as the float64 oracle; its finite numbers at rtol (the oracle's own two-pass float64 sums)."""
    for key, g in zip(("mean", "std", "error"), got):
        if ref[key] is None or g is None:
            continue
        g, r = np.asarray(g, np.float64).ravel(), np.asarray(ref[key], np.float64).ravel()
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what} {key}: NaN pattern {g} {r}"
        assert np.array_equal(np.isposinf(g), np.isposinf(r)) and np.array_equal(np.isneginf(g), np.isneginf(r)), f"{what} {key}: inf pattern {g} {r}"
        fin = np.isfinite(r)
        np.testing.assert_allclose(g[fin], r[fin], rtol=rtol, atol=1e-300, err_msg=f"{what} {key}")


def check_pair_special(device, x, sx, y, sy, mult, what):
    got = run_pair(device, x, sx, y, sy, mult)
    for g, r, kind in zip(got, oracle_pair(x, sx, y, sy, mult), ("abs", "rel")):
        assert_like_oracle(f"pair {what} {kind}", g, r, rtol=1e-9)


def check_pair_specials(device):
    """y = 0, x = y = 0, both stds 0 and the same frame on both sides, each at a lane's first element (pixel 0) and mid-block (pixel 40)."""
    rng = np.random.default_rng(10)
    for pix in (0, 40):
        for kind in ("y0", "xy0", "std0"):
            x, sx, y, sy = pair_frames(rng, 700, 3, nan=0.05)
            if kind == "y0":
                y[pix, 0], x[pix, 0] = 0.0, 0.5
            elif kind == "xy0":
                y[pix, 1], x[pix, 1] = 0.0, 0.0
            else:
                sx[pix, 2], sy[pix, 2], x[pix, 2], y[pix, 2] = 0.0, 0.0, 0.5, 0.6
            for with_std in (True, False):
                check_pair_special(device, x, sx if with_std else None, y, sy if with_std else None, 0.7, f"{kind} at pixel {pix} std={with_std}")
    x, sx, _, _ = pair_frames(rng, 700, 3)
    xt, st = T(x, device), T(sx, device)
    got = stats6(*eng(device, "pair_statistics", xt, st, xt, st, 1.0))      # the same frame on both sides: abs = 0 exactly
    for g, r, kind in zip(got, oracle_pair(x, sx, x, sx, 1.0), ("abs", "rel")):
        assert_like_oracle(f"pair same frame {kind}", g, r, rtol=1e-9)
    assert np.all(got[0][0] == 0.0) and np.all(got[0][1] == 0.0) and np.all(got[1][0] == 0.0) and np.all(got[1][1] == 0.0)


# ------------------------------------------------------------------------------------------------ hm_pairs_statistics
PAIRS_MAX, MAX_FRAMES = 16, nat.HM_MAX_FRAMES
PAIRS_STRIDE = 768 * 64                                                     # 49 152 elements per chunk row; an iteration (kPairUN = 2) is 98 304


def lds_ok(al16, n_frames, with_std, np_):
    """lds_ok() of hm_pairs_statistics: 16-byte aligned frames, at most two 16-byte items per thread, at most 21 KB-streams (3 stages in 64 KB)."""
    return al16 and n_frames <= 2 * np_ and n_frames * (2 if with_std else 1) <= 21


def launches(al16, n_frames, with_std, n_pairs):
    """-> per launch 'lds1' / 'lds2' (NI) or 'plain' (k_pairs_stats)."""
    out = []
    for p0 in range(0, n_pairs, PAIRS_MAX):
        np_ = min(PAIRS_MAX, n_pairs - p0)
        out.append(("lds1" if n_frames * 64 <= 64 * np_ else "lds2") if lds_ok(al16, n_frames, with_std, np_) else "plain")
    return out


def fused_end(al16, n_frames, with_std, n_pairs, n):
    """Elements below it are thresholded by the first launch's loader (whole iterations of every workgroup), the rest by k_thresholds."""
    grid = stat_grid(n, 64)
    stride, whole = grid * 64, 0
    while (grid - 1) * 64 + (2 * whole + 1) * stride + 64 <= n:
        whole += 1
    return 2 * stride * whole if lds_ok(al16, n_frames, with_std, min(n_pairs, PAIRS_MAX)) else 0


def all_pairs(n_frames, n_pairs):
    ps = [(i, j) for i in range(n_frames) for j in range(i + 1, n_frames)]
    assert ps
    return [(ps[k % len(ps)][0], ps[k % len(ps)][1], (0.1, 1.0, 7.3)[k % 3]) for k in range(n_pairs)]


def check_pairs(device, n_frames, n_pairs, n, C_, with_std, expect, thresholds=None, off8_frame=None, expect_fused=None, fam="pairs benign"):
    """n_frames frames of n elements, n_pairs pairs over them (multipliers 0.1, 1, 7.3 in turn); `expect`: the kernels of the launches."""
    assert n % C_ == 0
    al16 = off8_frame is None
    assert launches(al16, n_frames, with_std, n_pairs) == expect, (launches(al16, n_frames, with_std, n_pairs), expect)
    rng = np.random.default_rng(n_frames * 100 + n_pairs + n % 9973 + C_)
    vals, stds = [], []
    for f in range(0, n_frames, 2):
        x, sx, y, sy = pair_frames(rng, n // C_, C_)
        vals += [x, y]
        stds += [sx, sy]
    vals, stds = vals[:n_frames], stds[:n_frames]
    pairs = all_pairs(n_frames, n_pairs)
    tv = [offset_by_8(v, device) if f == off8_frame else T(v, device) for f, v in enumerate(vals)]
    ts = [T(s, device) for s in stds] if with_std else None
    if thresholds is not None:
        lo, hi = thresholds
        fe = fused_end(al16, n_frames, with_std, n_pairs, n)
        assert expect_fused is None or (0 < fe < n if expect_fused else fe == 0), (fe, n)
        thr = [orc.apply_thresholds(v, s, list(lo), list(hi)) for v, s in zip(vals, stds)]
        assert all(np.isnan(t).sum() > np.isnan(v).sum() + n // 50 for t, v in zip([t[0] for t in thr], vals))
        vals, stds = [t[0] for t in thr], [t[1] for t in thr]
    got = eng(device, "pairs_statistics", tv, ts, pairs, thresholds=thresholds)
    if thresholds is not None:
        for rep in range(2):                                                # in place, bit for bit - frames no pair references included; a second call changes nothing
            for f in range(n_frames):
                assert np.array_equal(to_np(tv[f]), vals[f], equal_nan=True), f"frame {f} after call {rep + 1}"
                assert ts is None or np.array_equal(to_np(ts[f]), stds[f], equal_nan=True), f"std {f} after call {rep + 1}"
            if rep == 0:
                again = eng(device, "pairs_statistics", tv, ts, pairs, thresholds=thresholds)
                for a, b in zip(got, again):
                    for da, db in zip(a, b):
                        for k in ("mean", "std"):
                            assert np.array_equal(to_np(da[k]), to_np(db[k]), equal_nan=True)
    hip = is_cuda(device)
    depth = stream_depth(hip, n, C_, 2, per=64) if hip else stream_depth(False, n, C_, 2)
    checked = sorted({0, len(pairs) // 2, len(pairs) - 1}) if thresholds is None else sorted({0, len(pairs) - 1})
    for p in checked:                                                       # (every pair's partials take the same path: the first, the last - in the last launch - and one between)
        i, j, mult = pairs[p]
        assert_pair(device, fam, f"pairs ({n_frames} frames, {n_pairs} pairs) n={n} C={C_} pair {p}", stats6(*got[p]), vals[i],
                    stds[i] if with_std else None, vals[j], stds[j] if with_std else None, mult, depth,
                    cap_depth=stream_depth(True, n, C_, 2, per=64))


IT = 2 * PAIRS_STRIDE                                                       # 98 304
# (n, id, r): n = 98 304 + 64 k + r with k chosen so that n stays a multiple of C = 3 (98 304 is one): r = 1: k = 2; r = C: k = 3; r = 63 (a
# 64-element chunk one lane short, ending on an odd element of the 16-byte loader): k = 3
PAIRS_SIZES = [(3 * 1000, "below one iteration", None), (IT, "one iteration exactly", 0), (IT + 64 * 2 + 1, "r = 1", 1), (IT + 64 * 3 + 3, "r = C", 3),
               (IT + 64 * 3 + 63, "r = 63", 63)]


def check_pairs_size(device, n, r, with_std):
    assert n % 3 == 0 and (r is None or (n >= IT and (n - IT) % 64 == r)), (n, r)
    check_pairs(device, 3, 3, n, 3, with_std, ["lds1"])


# (frames, pairs, with_std) -> launches
PAIRS_LIMITS = [
    (2, 1, True, ["lds2"]), (3, 3, True, ["lds1"]), (7, 16, True, ["lds1"]), (7, 18, True, ["lds1", "plain"]),
    (21, 16, False, ["lds2"]), (22, 16, False, ["plain"]), (10, 16, True, ["lds1"]), (11, 16, True, ["plain"]),
    (32, 16, False, ["plain"]), (32, 40, False, ["plain", "plain", "plain"]), (5, 2, True, ["plain"]),
]


# ------------------------------------------------------------------------------------------------ specials (channel / axis)
def check_extreme_weights_mid_block(device):
    """Stds 1e200 and 1e-200 in one line where a lane walks many elements, so the element of weight 1e200 arrives in a block whose shift is
    the running mean, not itself: k_axis_thread on (1, 45, 18) (KS = 2: the segment of odd positions holds both, at 21 and 23), and k_stats
    on 983 151 elements with the pair at lane 0's fifth and sixth element. Left in the block, its w d^2 = 1e198 absorbs the block's
    other terms in S2 and S2 - S1 q cancels down to what the other blocks hold (0.18 off on the std before acc_add() re-centred a block
    on an element that outweighs the lane's sum by 2^10)."""
    rng = np.random.default_rng(13)
    x, s3 = benign(rng, (1, 45, 18))
    x[0, 21, :], x[0, 23, :], s3[0, 21, :], s3[0, 23, :] = 0.25, 0.25, 1e200, 1e-200
    assert axis_geometry(1, 45, 18) == (False, 2, False)
    with np.errstate(all="ignore"):
        r3 = orc.dimension_statistics(x, s3, 1)
    assert np.all(r3["mean"] == 0.25) and np.all((0 < r3["std"]) & (r3["std"] < 1e-90))
    assert_like_oracle("axis (1, 45, 18), stds 1e200 and 1e-200 at positions 21 and 23", raw_axis(device, x, s3), r3)
    n, C_ = 5 * 196608 + 37 * 3, 3
    v, s = benign(rng, (n // C_, C_))
    for e, sd in ((4 * 196608, 1e200), (5 * 196608, 1e-200)):               # channel 0, lane 0 of workgroup 0: after the early fold
        v[e // C_, 0], s[e // C_, 0] = 0.25, sd
    with np.errstate(all="ignore"):
        ref = orc.dimension_statistics(v, s, 0)
    assert ref["mean"][0] == 0.25 and 0 < ref["std"][0] < 1e-90
    assert_like_oracle("channel, stds 1e200 and 1e-200 at a lane's fifth and sixth element", run_channel(device, v, s), ref)


def check_specials(device):
    """Each special once at a lane's first element (position 0 of its line) and once mid-block (position 21), weighted and not where it
    applies; the kernels of both layouts: channel statistics of (A, 3) and the row and thread axis kernels."""
    rng = np.random.default_rng(11)
    A = 45
    INF = np.inf

    def cases():
        for pos in (0, 21):
            for name, vv, ss in (("+inf", [INF], None), ("-inf", [-INF], None), ("both", [INF, -INF], None),
                                 ("std 0", None, [0.0]), ("std inf", None, [INF]), ("std 5e-324", None, [5e-324]), ("std 1e-310", None, [1e-310]),
                                 ("std 1e200 and 1e-200", None, [1e200, 1e-200])):
                v = rng.standard_normal((A, 3)) * 0.3 + 0.1
                s = 0.05 + 0.1 * rng.random((A, 3))
                v[rng.random((A, 3)) < 0.05] = np.nan
                for k, val in enumerate(vv or []):
                    v[pos + 2 * k, 1] = val
                for k, val in enumerate(ss or []):
                    s[pos + 2 * k, 1] = val
                    v[pos + 2 * k, 1] = 0.25
                yield f"{name} at {pos}", v, s
        v = rng.standard_normal((A, 3))
        s = 0.05 + 0.1 * rng.random((A, 3))
        v[:, 0] = INF                                                        # a line of only infinities
        v[:, 1] = np.nan                                                     # all-NaN
        v[:, 2] = np.nan
        v[17, 2] = 0.3                                                       # one counted element
        yield "only infinities | all NaN | one element", v, s
        v = np.full((A, 3), 0.1)                                             # all counted elements equal: M2 finishes at exactly 0
        v[5, 0] = np.nan
        yield "identical elements", v, np.full((A, 3), 0.07)

    for name, v, s in cases():
        for sw in (s, None):
            if sw is None and name.startswith("std"):
                continue
            if name == "identical elements":                                # finite lines: the reference and its bound; exactly 0 from the shifted sums
                got = run_channel(device, v, sw)
                assert_lines(device, "identical elements", f"channel {name} weighted={sw is not None}", got, channel_reference(v, sw), stream_depth(is_cuda(device), v.size, 3, 4))
                if is_cuda(device):
                    assert got[1][1] == 0.0 and got[1][2] == 0.0 and got[0][1] == 0.1, got          # not NaN, not 1e-17
                continue
            with np.errstate(all="ignore"):
                ref = orc.dimension_statistics(v, sw, 0)
            assert_like_oracle(f"channel {name} weighted={sw is not None}", run_channel(device, v, sw), ref)
            for x3, s3 in ((v.reshape(1, A, 3), None if sw is None else sw.reshape(1, A, 3)),                       # row kernel
                           (np.repeat(v.reshape(1, A, 3), 6, 2), None if sw is None else np.repeat(sw.reshape(1, A, 3), 6, 2))):   # thread kernel
                with np.errstate(all="ignore"):
                    r3 = orc.dimension_statistics(x3, s3, 1)
                assert_like_oracle(f"axis {x3.shape} {name} weighted={sw is not None}", raw_axis(device, x3, s3), r3)


# ------------------------------------------------------------------------------------------------ status codes
def check_status(device):
    """Every case returns before a launch; outputs keep their pre-fill. One table for both builds."""
    hip = is_cuda(device)
    OK, EINVAL, EALIGN = nat.HM_OK, nat.HM_EINVAL, nat.HM_EALIGN
    with backend(device) as (lib, stream):
        buf = torch.full((4096,), 0.5, dtype=torch.float64, device=device)
        out = torch.full((256,), 7.0, dtype=torch.float64, device=device)
        out_ks = torch.full((256,), 7.0, dtype=torch.float64, device=device)   # the one row of the table that computes (host build, see below)
        ws = torch.empty(max(8, int(nat.hip_lib.hm_pairs_statistics_workspace_bytes(2)) // 8), dtype=torch.float64, device=device)
        v, o, w, odd = buf.data_ptr(), out.data_ptr(), ws.data_ptr(), buf.data_ptr() + 4
        table = []
        chan = lambda val=v, sd=v, n=12, C_=3, o_=o, w_=w: lib.hm_channel_statistics(val, sd, n, C_, o_, w_, stream)          # noqa: E731
        pair = lambda x=v, sx=v, y=v, sy=v, n=12, C_=3, o_=o, w_=w: lib.hm_pair_statistics(x, sx, y, sy, 1.0, n, C_, o_, w_, stream)      # noqa: E731
        for name, f in (("channel", chan), ("pair", pair)):
            table += [(f"{name} n = 0", lambda f=f: f(n=0), EINVAL), (f"{name} C = 0", lambda f=f: f(C_=0), EINVAL), (f"{name} C = 5", lambda f=f: f(C_=5, n=10), EINVAL),
                      (f"{name} out NULL", lambda f=f: f(o_=None), EINVAL), (f"{name} workspace NULL", lambda f=f: f(w_=None), EINVAL),
                      (f"{name} n % C != 0", lambda f=f: f(n=13), EINVAL)]
        table += [("channel val NULL", lambda: chan(val=None), EINVAL), ("channel val misaligned", lambda: chan(val=odd), EALIGN),
                  ("channel std misaligned", lambda: chan(sd=odd), EALIGN), ("pair x NULL", lambda: pair(x=None), EINVAL), ("pair y NULL", lambda: pair(y=None), EINVAL),
                  ("pair x misaligned", lambda: pair(x=odd), EALIGN), ("pair sy misaligned", lambda: pair(sy=odd), EALIGN)]
        ax = lambda val=v, sd=v, dims=(2, 5, 3), w_=w, m_=o, b=o: lib.hm_axis_statistics(val, sd, *dims, m_, b + 512, b + 1024, w_, stream)       # noqa: E731
        ax2 = lambda val=v, sd=v, dims=(2, 3, 2, 5, 3), w_=w, m_=o: lib.hm_axis_statistics2(val, sd, *dims, m_, o + 512, o + 1024, w_, stream)   # noqa: E731
        big = (1 << 20, 1 << 20, 1 << 10)
        table += [("axis extent 0", lambda: ax(dims=(2, 0, 3)), EINVAL), ("axis extent -1", lambda: ax(dims=(-1, 5, 3)), EINVAL),
                  ("axis product 2^50", lambda: ax(dims=big), EINVAL), ("axis val NULL", lambda: ax(val=None), EINVAL), ("axis out NULL", lambda: ax(m_=None), EINVAL),
                  ("axis val misaligned", lambda: ax(val=odd), EALIGN), ("axis std misaligned", lambda: ax(sd=odd), EALIGN),
                  ("axis2 extent 0", lambda: ax2(dims=(2, 3, 0, 5, 3)), EINVAL), ("axis2 product 2^50", lambda: ax2(dims=(1 << 20, 1 << 10, 1 << 10, 1 << 5, 1 << 5)), EINVAL),
                  ("axis2 val NULL", lambda: ax2(val=None), EINVAL), ("axis2 val misaligned", lambda: ax2(val=odd), EALIGN), ("axis2 std misaligned", lambda: ax2(sd=odd), EALIGN)]
        # KS > 1 ((1, 320, 16): 20 segments) with a NULL workspace. The host build needs none (its workspace size is 0): it computes.
        assert axis_geometry(1, 320, 16)[1] == 20
        table += [("axis KS > 1, workspace NULL", lambda: ax(dims=(1, 320, 16) if hip else (1, 20, 16), w_=None, m_=out_ks.data_ptr(), b=out_ks.data_ptr()),
                   EINVAL if hip else OK)]
        assert lib.hm_axis_statistics_workspace_bytes(*big) == 0 and lib.hm_axis_statistics2_workspace_bytes(1 << 20, 1 << 10, 1 << 10, 1 << 5, 1 << 5) == 0

        def pairs(frames=(v, v + 512 * 8), sds=(v + 1024 * 8, v + 1536 * 8), n_frames=None, pi=(0,), pj=(1,), n_pairs=None, n=12, C_=3, lower=None, upper=None, o_=o, w_=w):
            nf = len(frames) if n_frames is None else n_frames
            arr = lambda ps: None if ps is None else C.cast((C.c_void_p * max(1, len(ps)))(*ps), C.POINTER(C.c_void_p))        # noqa: E731
            lim = lambda q: None if q is None else (C.c_double * len(q))(*q)     # noqa: E731
            npairs = len(pi) if n_pairs is None else n_pairs
            return lib.hm_pairs_statistics(arr(frames), arr(sds), nf, (C.c_int32 * max(1, len(pi)))(*pi), (C.c_int32 * max(1, len(pj)))(*pj),
                                           (C.c_double * max(1, len(pi)))(*([1.0] * len(pi))), npairs, n, C_, lim(lower), lim(upper), o_, w_, stream)
        many = tuple([v] * (MAX_FRAMES + 1))
        table += [("pairs n = 0", lambda: pairs(n=0), EINVAL), ("pairs C = 5", lambda: pairs(C_=5, n=10), EINVAL), ("pairs n % C != 0", lambda: pairs(n=13), EINVAL),
                  ("pairs out NULL", lambda: pairs(o_=None), EINVAL), ("pairs workspace NULL", lambda: pairs(w_=None), EINVAL),
                  ("pairs n_pairs = 0", lambda: pairs(n_pairs=0), EINVAL), ("pairs n_frames = 0", lambda: pairs(n_frames=0), EINVAL),
                  ("pairs n_frames = HM_MAX_FRAMES + 1", lambda: pairs(frames=many, sds=None), EINVAL),
                  ("pairs a frame NULL", lambda: pairs(frames=(v, None)), EINVAL), ("pairs a std NULL", lambda: pairs(sds=(v, None)), EINVAL),
                  ("pairs a frame misaligned", lambda: pairs(frames=(v, odd)), EALIGN), ("pairs a std misaligned", lambda: pairs(sds=(odd, v)), EALIGN),
                  ("pairs lower without upper", lambda: pairs(lower=(0.0,) * 3), EINVAL), ("pairs upper without lower", lambda: pairs(upper=(1.0,) * 3), EINVAL),
                  ("pairs index = n_frames", lambda: pairs(pj=(2,)), EINVAL), ("pairs index -1", lambda: pairs(pi=(-1,)), EINVAL)]
        wrong = [(name, rc, want) for name, rc, want in ((name, call(), want) for name, call, want in table) if rc != want]
        assert not wrong, f"(case, returned, expected): {wrong}"
        if hip:
            torch.cuda.synchronize()
        assert np.all(to_np(out) == 7.0), "an entry point that returned an error wrote to its outputs (mean, std or error)"
        assert hip == bool(np.all(to_np(out_ks) == 7.0))
        assert pairs() == OK and chan() == OK and pair() == OK and ax() == OK and ax2() == OK      # the table's valid call is valid
    return len(table)


# ================================================================================================ the host build
DEV = "cpu"
STD = pytest.mark.parametrize("weighted", [False, True])


def test_reference_is_the_oracle():
    """line_reference / pair_lines against oracle.dimension_statistics / compute_difference on one benign case at 1e-13: the new reference
    stays tied to the oracle the golden fixtures pin."""
    rng = np.random.default_rng(1)
    v, s = benign(rng, (500, 3))
    for sw in (s, None):
        o = orc.dimension_statistics(v, sw, 0)
        r = channel_reference(v, sw)
        np.testing.assert_allclose(r["m"].astype(np.float64), o["mean"], rtol=1e-13)
        np.testing.assert_allclose(r["sigma"].astype(np.float64), o["std"], rtol=1e-13)
        if sw is not None:
            np.testing.assert_allclose(r["err"].astype(np.float64), o["error"], rtol=1e-13)
    x, sx, y, sy = pair_frames(rng, 500, 3)
    for (v_, w_, s_), o in zip(pair_lines(x, sx, y, sy, 0.7), oracle_pair(x, sx, y, sy, 0.7)):
        r = line_reference(v_, w_, s_, r_all=True)
        for k, ok in (("m", "mean"), ("sigma", "std"), ("err", "error")):
            np.testing.assert_allclose(r[k].astype(np.float64), o[ok], rtol=1e-13)
    ad, ads, rd, rds = orc.compute_difference(x, sx, y, sy, 0.7)
    (av, aw, as_), (rv, rw, rs) = pair_lines(x, sx, y, sy, 0.7)
    for mine, theirs in ((av, ad), (as_, ads), (rv, rd), (rs, rds), (1 / aw, ads)):
        np.testing.assert_allclose(mine.T.astype(np.float64), theirs, rtol=1e-13)


def test_geometry_restated_here_matches_the_library():
    """The grids restated in this module against what the library's entry points expose."""
    assert int(nat.hip_lib.hm_channel_statistics_workspace_bytes()) == 8 * STAT_BLOCKS * 4 * 6
    assert int(nat.hip_lib.hm_pairs_statistics_workspace_bytes(16)) == 8 * STAT_BLOCKS * 16 * 4 * 2 * 6
    assert stat_grid(200) == 12 and stat_grid(196608) == 768 and stat_grid(98304, 64) == 768 and stat_grid(3000, 64) == 48
    for table in (AXIS_THREAD, AXIS_ROW, AXIS_ROW_LONG):
        for shape, expect in table.items():
            assert axis_geometry(*shape) == expect, (shape, axis_geometry(*shape), expect)
    for shape, expect in AXIS2.items():
        o1, A, i1, R, row, KS, tree = axis2_geometry(*shape)
        assert (shape[1] >= shape[3], row, KS, tree) == expect, (shape, (shape[1] >= shape[3], row, KS, tree), expect)
    check_axis_empty_segments(DEV)
    # the folds the cases are built for: two mid-stream folds at the two-fold size; 130-element chains fold twice and keep a tail
    assert stream_depth(True, TWO_FOLDS + 3 * 3 * 37, 3, 4)["folds"] == 2 + 2 and stream_depth(True, TWO_FOLDS + 3 * 3 * 37, 3, 8)["folds"] == 2 + 2
    assert stream_depth(True, 3145728 + 2 * IT + 37 * 3, 3, 2, per=64)["folds"] == 2 + 1
    assert axis_depth(True, 1, 33280, 16)["folds"] == 2 + 2 and axis_depth(True, 1, 33280, 16)["wall"] == 130


@STD
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_channel_sizes(C_, weighted):
    for n in channel_sizes(C_, weighted):
        check_channel(DEV, n, C_, weighted)


@STD
def test_channel_offset_view(weighted):
    check_channel(DEV, 3 * 4099, 3, weighted, off8=True)


@STD
def test_channel_offset_family(weighted):
    check_channel(DEV, 3 * 65599, 3, weighted, fam="offset")


def test_channel_heavy_tailed():
    check_channel_heavy(DEV)


def test_negative_stds():
    check_channel_negative(DEV)


def test_specials():
    check_specials(DEV)


def test_extreme_weights_mid_block():
    check_extreme_weights_mid_block(DEV)


@STD
@pytest.mark.parametrize("shape", list(AXIS_THREAD), ids=str)
def test_axis_thread(shape, weighted):
    check_axis(DEV, shape, weighted, AXIS_THREAD[shape], with_err=with_err_for(shape))


@STD
@pytest.mark.parametrize("shape", list(AXIS_ROW), ids=str)
def test_axis_row(shape, weighted):
    check_axis(DEV, shape, weighted, AXIS_ROW[shape], with_err=with_err_for(shape))


@STD
def test_axis_offset_family_and_view(weighted):
    check_axis(DEV, (1, 33280, 16), weighted, AXIS_THREAD[(1, 33280, 16)], fam="offset")
    check_axis(DEV, (1, 6000, 15), weighted, AXIS_ROW[(1, 6000, 15)], fam="offset")
    check_axis(DEV, (3, 200, 40), weighted, AXIS_THREAD[(3, 200, 40)], off8=True)
    check_axis(DEV, (1024, 33, 3), weighted, AXIS_ROW[(1024, 33, 3)], off8=True)


def test_axis_heavy_tailed():
    check_axis_heavy(DEV)


@STD
@pytest.mark.parametrize("shape", list(AXIS2), ids=str)
def test_axis2(shape, weighted):
    check_axis2(DEV, shape, weighted, AXIS2[shape])


@pytest.mark.parametrize("SX,SY", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("C_", [1, 3, 4])
def test_pair_sizes(C_, SX, SY):
    for k, n in enumerate(pair_sizes(C_, SX or SY)):
        check_pair(DEV, n, C_, SX, SY, (0.1, 0.1, 1.0, 7.3, 1.0)[k])


def test_pair_offset_view():
    check_pair(DEV, 3 * 4099, 3, True, True, 7.3, off8=True)


def test_pair_heavy_tailed():
    check_pair_heavy(DEV)


def test_pair_specials():
    check_pair_specials(DEV)
    check_pair_one_special_lane(DEV)


@pytest.mark.parametrize("with_std", [False, True])
@pytest.mark.parametrize("n,what,r", PAIRS_SIZES, ids=[w for _, w, _ in PAIRS_SIZES])
def test_pairs_sizes(n, what, r, with_std):
    check_pairs_size(DEV, n, r, with_std)


@pytest.mark.parametrize("frames,pairs,with_std,expect", PAIRS_LIMITS)
def test_pairs_limits(frames, pairs, with_std, expect):
    check_pairs(DEV, frames, pairs, IT + 64 * 3 + 3, 3, with_std, expect)


def test_pairs_unaligned_frame():
    check_pairs(DEV, 3, 3, IT + 64 * 3 + 3, 3, True, ["plain"], off8_frame=1)


THR_N = ((IT + 64 * 5 + 7) // 12) * 12                                      # one whole iteration for every workgroup (fused), then a tail (k_thresholds)
THRESHOLDS = {1: ([0.6], [1.1]), 2: ([0.6, -np.inf], [np.inf, 1.0]), 3: ([0.55, -np.inf, 0.6], [1.15, np.inf, 1.05]), 4: ([0.6, 0.55, -np.inf, 0.65], [1.1, 1.0, np.inf, np.inf])}


@pytest.mark.parametrize("with_std", [False, True])
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_pairs_thresholds(C_, with_std):
    """Fused into the loader (elements on both sides of fused_end; frame 3 is in no pair), k_thresholds only (small n; an unaligned frame; lds_ok false)."""
    n = THR_N
    check_pairs(DEV, 4, 2, n, C_, with_std, ["lds2"], THRESHOLDS[C_], expect_fused=True, fam="pairs thresholds")
    check_pairs(DEV, 4, 3, 12 * 250, C_, with_std, ["lds2"], THRESHOLDS[C_], expect_fused=False, fam="pairs thresholds")
    check_pairs(DEV, 4, 3, n, C_, with_std, ["plain"], THRESHOLDS[C_], off8_frame=2, expect_fused=False, fam="pairs thresholds")
    check_pairs(DEV, 5, 2, n, C_, with_std, ["plain"], THRESHOLDS[C_], expect_fused=False, fam="pairs thresholds")


def check_thresholds_on_a_limit(device):
    """The test is < / >: a value exactly on a limit stays; -inf / +inf limits keep everything of their channel."""
    rng = np.random.default_rng(12)
    n, C_ = THR_N, 3
    x, sx, y, sy = pair_frames(rng, n // C_, C_)
    x[::7, 0], x[3::7, 0] = 0.6, 1.1
    tv, ts = [T(x, device), T(y, device)], [T(sx, device), T(sy, device)]
    eng(device, "pairs_statistics", tv, ts, [(0, 1, 1.0)], thresholds=([0.6, -np.inf, 0.55], [1.1, np.inf, 1.15]))
    got = to_np(tv[0])
    assert np.all(got[::7, 0] == 0.6) and np.all(got[3::7, 0] == 1.1) and np.array_equal(got[:, 1], x[:, 1], equal_nan=True)
    ref = orc.apply_thresholds(x, sx, [0.6, -np.inf, 0.55], [1.1, np.inf, 1.15])
    assert np.array_equal(got, ref[0], equal_nan=True) and np.array_equal(to_np(ts[0]), ref[1], equal_nan=True)


def test_thresholds_keep_values_on_a_limit():
    check_thresholds_on_a_limit(DEV)


def test_status_codes():
    assert check_status(DEV) >= 48
