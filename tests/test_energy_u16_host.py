"""The ICRF-calibration energy on uint16 DN stacks of 9- to 16-bit cameras (hm_linearity_energy_u16, engine.linearity_energy(...,
bit_depth=b), icrf_calibration up to calibration(..., bit_depth=b)) on the HOST build. The checks are functions of a device name:
tests/test_gpu_energy_u16.py runs the same ones on the MI355X.

What is compared, and with what:
    embedding   an 8-bit problem embedded at depth b (DN << (b - 8), the 256 entries at rows k << (b - 8), every other row NaN, limits
                shifted alike) gives hm_linearity_energy's out_energy and out_pairs as integer bit patterns, in every placement of the
                candidate's row (variant 0, 1 where the row fits LDS, 2), the placements equal to each other.
    oracle      oracle/hdr_oracle.py's analyze_linearity_pairs and energy_function (they index icrf[dn]: any depth) on DNs uniform over the
                full range, rtol = 1e-12 - the tolerance of the 8-bit check (tests/test_gpu_producers.py::test_energy_vs_oracle). The
                oracle's pair results must hold no NaN for these inputs (asserted), so equal_nan hides nothing.
    The argument rules are called through ctypes on both builds: every refusal returns before anything is launched, so the device
    library answers them on host pointers."""
import ctypes as C

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from camera_linearity_amd import icrf_calibration as ic
from oracle import hdr_oracle as orc

# (X, Y, N, B): pixel-major; pixel-major because P <= 16384; P = 16 899 > 16384: a lone candidate runs pair-major over 17 chunks;
# N > 8: pair-major; HM_MAX_FRAMES; a single pixel
SHAPES = [(27, 27, 7, 8), (27, 27, 7, 1), (131, 129, 3, 1), (33, 31, 9, 4), (5, 4, 32, 2), (1, 1, 2, 1)]
EMBED_DEPTHS = [9, 12, 14, 15, 16]
ORACLE_DEPTHS = [10, 12, 14, 16]
MODES = [(False, True), (False, False), (True, True), (True, False)]          # (with_std, use_relative)
LDS_MAX_DEPTH = 14                                                            # hm_calibration_rules.h: energy_u16_row_fits_lds


def eng(dev):
    """engine on a device stack, the host build of the same functions on a host stack"""
    return engine if torch.device(dev).type == "cuda" else ic._engine_for(torch.zeros(1))


def T(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def variants(depth):
    return (0, 1, 2) if depth <= LDS_MAX_DEPTH else (0, 2)


def bits_of(t):
    return t.cpu().numpy().view(np.int64)


def pixel_major(N, B, P):
    """energy_pixel_major of csrc/hm_energy_dev.h"""
    return N <= 8 and (B >= 8 or P <= 16384)


def kernel_of(P, N, B, with_std, depth, variant):
    """the DEVICE library's name of the kernel of such a call (hm_linearity_energy_u16_describe launches nothing: any machine)"""
    buf = C.create_string_buffer(128)
    assert nat.hip_lib.hm_linearity_energy_u16_describe(P, N, B, int(with_std), depth, variant, buf, len(buf)) == nat.HM_OK
    return buf.value.decode()


# ------------------------------------------------------------------------------------------------ 1: embedding
def problem_8bit(X, Y, N, B, seed):
    rng = np.random.default_rng(seed)
    dn = rng.integers(0, 256, (X, Y, N), dtype=np.uint8)
    sd = 0.004 * (1 + rng.random((X, Y, N)))
    t = 1e-3 * 1.3 ** np.arange(N)
    icrfs = np.linspace(0, 1, 256)[None, :] ** (1.0 + 0.4 * np.arange(B))[:, None]
    icrfs[:, -1] = 1.0
    return dn, sd, t, icrfs


def embed(dn, icrfs, depth):
    s = depth - 8
    wide = np.full((icrfs.shape[0], 2 ** depth), np.nan)
    wide[:, np.arange(256) << s] = icrfs
    return (dn.astype(np.uint16) << s), wide, s


def check_embedding(dev, shape, depth):
    X, Y, N, B = shape
    dn, sd, t, icrfs = problem_8bit(X, Y, N, B, 100 * X + N)
    dn16, wide, s = embed(dn, icrfs, depth)
    e = eng(dev)
    d8, d16, sdt, lut16 = T(dn, dev), T(dn16, dev), T(sd, dev), T(wide, dev)
    for with_std, rel in MODES:
        sd_ = sdt if with_std else None
        e8, p8 = e.linearity_energy(d8, sd_, t, icrfs, 5, 250, None, rel, return_pairs=True)
        for v in variants(depth):
            e16, p16 = e.linearity_energy(d16, sd_, t, lut16, 5 << s, 250 << s, None, rel, return_pairs=True, bit_depth=depth, variant=v)
            assert np.array_equal(bits_of(e16), bits_of(e8)), (shape, depth, with_std, rel, v)
            assert np.array_equal(bits_of(p16), bits_of(p8)), (shape, depth, with_std, rel, v)
            if torch.device(dev).type == "cuda":
                k = e.energy_kernel(X * Y, N, B, with_std, depth, v)
                assert k.startswith("k_energy_pixel_u16<" if pixel_major(N, B, X * Y) else "k_energy_partial_u16<"), k
                assert v == 0 or ("lut=lds" in k) == (v == 1), k


@pytest.mark.parametrize("depth", EMBED_DEPTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_embedding_bit_patterns(shape, depth):
    check_embedding("cpu", shape, depth)


def test_embedding_holds_in_the_oracle():
    """the embedding itself, on the NumPy oracle: the pair results of the embedded problem are those of the 8-bit one exactly"""
    X, Y, N, B = SHAPES[0]
    dn, sd, t, icrfs = problem_8bit(X, Y, N, B, 3)
    for depth in (9, 12, 16):
        dn16, wide, s = embed(dn, icrfs, depth)
        for with_std, rel in MODES:
            sd_ = sd if with_std else None
            a = orc.analyze_linearity_pairs(icrfs[1][dn], sd_, icrfs[1][5], icrfs[1][250], rel, t)
            b = orc.analyze_linearity_pairs(wide[1][dn16], sd_, wide[1][5 << s], wide[1][250 << s], rel, t)
            assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_the_cases_reach_all_four_kernels():
    """(geometry, placement): the embedding cases name, through _describe, both kernel families in both placements of the row"""
    seen = set()
    for X, Y, N, B in SHAPES:
        for depth in EMBED_DEPTHS:
            for v in variants(depth):
                k = kernel_of(X * Y, N, B, True, depth, v)
                assert f"bits={depth}" in k and "std=1" in k
                assert k.startswith("k_energy_pixel_u16<") == pixel_major(N, B, X * Y), k
                if v:
                    assert ("lut=lds" in k) == (v == 1), k
                seen.add((k.split("<")[0], "lds" if "lut=lds" in k else "global"))
    assert seen == {(f, p) for f in ("k_energy_pixel_u16", "k_energy_partial_u16") for p in ("lds", "global")}
    assert kernel_of(27 * 27, 7, 8, True, 12, 1) == "k_energy_pixel_u16<N=7,std=1,lut=lds,bits=12>"
    assert kernel_of(33 * 31, 9, 4, False, 16, 0) == "k_energy_partial_u16<std=0,lut=global,bits=16>(N=9)"


# ------------------------------------------------------------------------------------------------ 2: the oracle at full range
def problem_full_range(X, Y, N, B, depth, seed, inside=False):
    rng = np.random.default_rng(seed)
    n = 2 ** depth
    lower, upper = int(round(0.02 * (n - 1))), int(round(0.98 * (n - 1)))
    dn = (rng.integers(lower, upper + 1, (X, Y, N)) if inside else rng.integers(0, n, (X, Y, N))).astype(np.uint16)
    sd = 0.004 * (1 + rng.random((X, Y, N)))
    t = 1e-3 * 1.3 ** np.arange(N)
    icrfs = np.linspace(0, 1, n)[None, :] ** (2.0 + 0.25 * np.arange(B))[:, None]       # row 0: linspace ** 2
    icrfs[:, -1] = 1.0
    return dn, sd, t, icrfs, lower, upper


def against_oracle(dev, dn, sd, t, icrfs, lower, upper, depth, rel=True, variant=0, no_nan=True):
    e, pairs = eng(dev).linearity_energy(T(dn, dev), T(sd, dev), t, icrfs, lower, upper, None, rel, return_pairs=True, bit_depth=depth,
                                         variant=variant)
    for b in range(len(icrfs)):
        ref = orc.analyze_linearity_pairs(icrfs[b][dn], sd, icrfs[b][lower], icrfs[b][upper], rel, t)
        assert not (no_nan and np.isnan(ref).any()), "the oracle's pair results must hold no NaN here"
        np.testing.assert_allclose(pairs[b].cpu().numpy(), ref, rtol=1e-12, equal_nan=True)
        if rel:
            np.testing.assert_allclose(float(e[b]), orc.energy_function(icrfs[b], dn, sd, lower, upper, t), rtol=1e-12)
    return e, pairs


def check_oracle(dev, shape, depth, with_std):
    X, Y, N, B = shape
    dn, sd, t, icrfs, lower, upper = problem_full_range(X, Y, N, B, depth, 10 * X + N + depth, inside=(X * Y == 1))
    for v in variants(depth)[1:]:
        against_oracle(dev, dn, sd if with_std else None, t, icrfs, lower, upper, depth, variant=v)


@pytest.mark.parametrize("with_std", [False, True])
@pytest.mark.parametrize("depth", ORACLE_DEPTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_oracle(shape, depth, with_std):
    check_oracle("cpu", shape, depth, with_std)


# ------------------------------------------------------------------------------------------------ 3: the index convention
def check_stray_high_bits(dev, depth):
    X, Y, N, B = 27, 27, 7, 8
    dn, sd, t, icrfs, lower, upper = problem_full_range(X, Y, N, B, depth, depth)
    stray = (dn | (np.random.default_rng(1).integers(0, 2 ** (16 - depth), dn.shape) << depth)).astype(np.uint16)
    assert (stray != dn).any() and np.array_equal(stray & (2 ** depth - 1), dn)
    for X_, B_ in ((27, 8), (131, 1)):                                     # both geometries
        a, b, s = np.resize(dn, (X_, Y, N)), np.resize(stray, (X_, Y, N)), np.resize(sd, (X_, Y, N))
        for v in variants(depth)[1:]:
            want = eng(dev).linearity_energy(T(a, dev), T(s, dev), t, icrfs[:B_], lower, upper, None, True, True, bit_depth=depth, variant=v)
            got = eng(dev).linearity_energy(T(b, dev), T(s, dev), t, icrfs[:B_], lower, upper, None, True, True, bit_depth=depth, variant=v)
            assert np.array_equal(bits_of(got[0]), bits_of(want[0])) and np.array_equal(bits_of(got[1]), bits_of(want[1]))


@pytest.mark.parametrize("depth", [9, 12, 15])
def test_stray_high_bits_are_masked(depth):
    check_stray_high_bits("cpu", depth)


# ------------------------------------------------------------------------------------------------ 4: edges
def check_limits_at_the_ends(dev, depth):
    dn, sd, t, icrfs, _, _ = problem_full_range(27, 27, 3, 2, depth, 5)
    for rel in (True, False):
        against_oracle(dev, dn, sd, t, icrfs, 0, 2 ** depth - 1, depth, rel=rel, no_nan=False)


def check_all_outside(dev, depth):
    n = 2 ** depth
    dn = np.random.default_rng(2).integers(0, n // 4, (9, 9, 3)).astype(np.uint16)
    icrf = np.linspace(0, 1, n)[None]
    for v in variants(depth):
        e, p = eng(dev).linearity_energy(T(dn, dev), None, [1.0, 2.0, 4.0], icrf, n // 2, n - 1, None, True, True, bit_depth=depth, variant=v)
        assert np.isposinf(e.cpu().numpy()).all() and np.isnan(p.cpu().numpy()).all()


def check_valid_rows(dev, depth):
    dn, sd, t, icrfs, lower, upper = problem_full_range(27, 27, 7, 8, depth, 8)
    valid = np.array([1, 0, 1, 1, 0, 0, 1, 1], dtype=bool)
    for v in variants(depth):
        full = eng(dev).linearity_energy(T(dn, dev), T(sd, dev), t, icrfs, lower, upper, None, True, True, bit_depth=depth, variant=v)
        e, p = eng(dev).linearity_energy(T(dn, dev), T(sd, dev), t, icrfs, lower, upper, valid, True, True, bit_depth=depth, variant=v)
        e, p = e.cpu().numpy(), p.cpu().numpy()
        assert np.isposinf(e[~valid]).all() and np.isnan(p[~valid]).all()
        assert np.array_equal(e[valid].view(np.int64), bits_of(full[0])[valid]) and np.array_equal(p[valid].view(np.int64), bits_of(full[1])[valid])


def check_geometry_switch(dev, depth):
    """7 candidates against 8 on a stack of more than 16 384 pixels: pair-major against pixel-major, both at the oracle's tolerance"""
    X, Y, N = 131, 129, 3
    dn, sd, t, icrfs, lower, upper = problem_full_range(X, Y, N, 8, depth, 9)
    assert kernel_of(X * Y, N, 7, True, depth, 0).startswith("k_energy_partial_u16<")
    assert kernel_of(X * Y, N, 8, True, depth, 0).startswith("k_energy_pixel_u16<")
    for B in (7, 8):
        against_oracle(dev, dn, sd, t, icrfs[:B], lower, upper, depth)


def check_pixel_counts(dev, depth, X, Y):
    dn, sd, t, icrfs, lower, upper = problem_full_range(X, Y, 3, 2, depth, X)
    for v in variants(depth)[1:]:
        against_oracle(dev, dn, sd, t, icrfs, lower, upper, depth, variant=v)


def check_odd_element_offset(dev, depth):
    X, Y, N = 9, 7, 3
    dn, sd, t, icrfs, lower, upper = problem_full_range(X, Y, N, 2, depth, 4)
    flat = torch.zeros(X * Y * N + 1, dtype=torch.int16, device=dev)
    flat[1:] = T(dn.view(np.int16).reshape(-1), dev)
    view = flat.view(torch.uint16)[1:].view(X, Y, N)
    assert view.data_ptr() % 4 == 2 and view.is_contiguous()
    want = eng(dev).linearity_energy(T(dn, dev), T(sd, dev), t, icrfs, lower, upper, None, True, True, bit_depth=depth)
    got = eng(dev).linearity_energy(view, T(sd, dev), t, icrfs, lower, upper, None, True, True, bit_depth=depth)
    assert np.array_equal(bits_of(got[0]), bits_of(want[0])) and np.array_equal(bits_of(got[1]), bits_of(want[1]))


EDGE_CHECKS = {
    "limits at 0 and 2^b - 1": lambda dev: [check_limits_at_the_ends(dev, d) for d in (10, 16)],
    "every DN outside the limits": lambda dev: [check_all_outside(dev, d) for d in (9, 14, 16)],
    "valid = 0 rows": lambda dev: [check_valid_rows(dev, d) for d in (12, 15)],
    "7 against 8 candidates": lambda dev: check_geometry_switch(dev, 12),
    "P = 1024": lambda dev: check_pixel_counts(dev, 12, 32, 32),
    "P = 1025": lambda dev: check_pixel_counts(dev, 12, 41, 25),
    "P = 257": lambda dev: check_pixel_counts(dev, 13, 257, 1),
    "dn at an odd element offset": lambda dev: [check_odd_element_offset(dev, d) for d in (12, 16)],
}


@pytest.mark.parametrize("name", list(EDGE_CHECKS))
def test_edges(name):
    EDGE_CHECKS[name]("cpu")


# ------------------------------------------------------------------------------------------------ 5: the rules, both builds
def _rule_call(lib, depth=12, **over):
    """hm_linearity_energy_u16 on host buffers of 8 pixels x 2 frames, 2 candidates, with the faults of `over`; -> status.
    Only for calls that return before anything is launched (or, on the host build, any call)."""
    n = 2 ** depth
    keep = dict(dn=np.zeros(2 * 8 * 2 + 1, np.uint16), icrf=np.tile(np.linspace(0, 1, n), 2), out_pairs=np.zeros(2), out_energy=np.zeros(2),
                ws=np.zeros(64))
    a = dict(dn=keep["dn"].ctypes.data, std=None, exposures=(C.c_double * 33)(*[1e-3 * 1.5 ** i for i in range(33)]), icrf=keep["icrf"].ctypes.data,
             valid=None, n_candidates=2, lower=5, upper=n - 6, use_relative=1, n_pixels=8, n_frames=2, bit_depth=depth, variant=0,
             out_pairs=keep["out_pairs"].ctypes.data, out_energy=keep["out_energy"].ctypes.data, workspace=keep["ws"].ctypes.data, stream=None)
    a.update(over)
    return lib.hm_linearity_energy_u16(*a.values())


EINVAL, ESHAPE, EUNSUP, EALIGN, OK = nat.HM_EINVAL, nat.HM_ESHAPE, nat.HM_EUNSUPPORTED, nat.HM_EALIGN, nat.HM_OK
ODD = "an odd address"                                                        # (replaced by one inside the test)
# in the header's order; every fault alone
RULE_FAULTS = [
    (1, dict(n_candidates=-1), EINVAL), (1, dict(n_pixels=-1), EINVAL), (1, dict(bit_depth=8), EINVAL), (1, dict(bit_depth=17), EINVAL),
    (1, dict(variant=-1), EINVAL), (1, dict(variant=3), EINVAL),
    (2, dict(n_frames=1), ESHAPE), (2, dict(n_frames=33), ESHAPE),
    (3, dict(lower=-1), EINVAL), (3, dict(lower=4096), EINVAL), (3, dict(upper=-1), EINVAL), (3, dict(upper=4096), EINVAL),
    (4, dict(n_candidates=0), OK),
    (5, dict(n_candidates=65536), EUNSUP), (5, dict(bit_depth=15, variant=1), EUNSUP), (5, dict(bit_depth=16, variant=1), EUNSUP),
    (6, dict(dn=None), EINVAL), (6, dict(exposures=None), EINVAL), (6, dict(icrf=None), EINVAL), (6, dict(out_energy=None), EINVAL),
    (7, dict(dn=ODD), EALIGN),
]


def _libs():
    return [("device", nat.hip_lib), ("host", nat.host_lib())]


def _resolve(lib_over):
    if lib_over.get("dn") == ODD:
        lib_over = dict(lib_over, dn=_ODD_BUF.ctypes.data + 1)
    return lib_over


_ODD_BUF = np.zeros(64, np.uint16)


def test_rules_every_status_in_order():
    for name, lib in _libs():
        for stage, over, code in RULE_FAULTS:
            assert _rule_call(lib, **_resolve(over)) == code, (name, over)
        # an earlier rule wins over a later one broken in the same call
        for (s1, o1, c1) in RULE_FAULTS:
            for (s2, o2, c2) in RULE_FAULTS:
                if s1 < s2 and c1 != c2 and not set(o1) & set(o2) and not (s1 == 3 and "bit_depth" in o2):     # (a limit of 4096 is one of 15 bits)
                    assert _rule_call(lib, **_resolve({**o1, **o2})) == c1, (name, o1, o2)
    # the limits follow the depth
    for name, lib in _libs():
        assert _rule_call(lib, depth=9, n_candidates=0, upper=511) == OK and _rule_call(lib, depth=9, upper=512) == EINVAL
        assert _rule_call(lib, depth=16, n_candidates=0, upper=65535) == OK and _rule_call(lib, depth=16, upper=65536) == EINVAL
    # the device build's own: a NULL workspace comes last
    assert _rule_call(nat.hip_lib, workspace=None) == EINVAL
    assert _rule_call(nat.hip_lib, workspace=None, dn=_ODD_BUF.ctypes.data + 1) == EALIGN


def test_rules_no_candidates_with_null_pointers():
    for name, lib in _libs():
        assert _rule_call(lib, n_candidates=0, dn=None, exposures=None, icrf=None, out_energy=None, out_pairs=None, workspace=None) == OK, name


def test_variant_1_at_15_bits_is_not_implemented():
    dn = torch.zeros((3, 3, 2), dtype=torch.uint16)
    with pytest.raises(NotImplementedError):
        eng("cpu").linearity_energy(dn, None, [1.0, 2.0], np.linspace(0, 1, 2 ** 15)[None], 5, 2 ** 15 - 6, bit_depth=15, variant=1)
    for name, lib in _libs():
        buf = C.create_string_buffer(64)
        assert lib.hm_linearity_energy_u16_describe(9, 2, 1, 0, 15, 1, buf, len(buf)) == EUNSUP, name
        assert lib.hm_linearity_energy_u16_describe(9, 2, 1, 0, 14, 1, buf, len(buf)) == OK and buf.value, name
        assert lib.hm_linearity_energy_u16_describe(9, 2, 1, 0, 14, 1, None, 0) == EINVAL, name


def test_workspace_size_is_the_8_bit_entry_s():
    """the chunk count, and with it the workspace, is a function of (n_pixels, n_frames, n_candidates) alone"""
    assert nat.hip_lib.hm_linearity_energy_workspace_bytes(16899, 3, 1) == 1 * 3 * 17 * 16


# ------------------------------------------------------------------------------------------------ 6: the Python surface
def check_python_surface(dev):
    e = eng(dev)
    t = [1.0, 2.0]
    u16 = torch.zeros((3, 3, 2), dtype=torch.uint16, device=dev)
    u8 = torch.zeros((3, 3, 2), dtype=torch.uint8, device=dev)
    row12, row8 = np.linspace(0, 1, 4096)[None], np.linspace(0, 1, 256)[None]
    with pytest.raises(ValueError, match="bit_depth"):
        e.linearity_energy(u16, None, t, row12, 5, 250)                                        # uint16 without a depth
    for bad in (8, 17, 12.0, True):
        with pytest.raises(ValueError, match="bit_depth"):
            e.linearity_energy(u16, None, t, row12, 5, 250, bit_depth=bad)
    with pytest.raises(ValueError, match="bit_depth"):
        e.linearity_energy(u8, None, t, row8, 5, 250, bit_depth=12)                            # a depth with uint8 DNs
    with pytest.raises(ValueError, match="bit_depth"):
        e.linearity_energy(u8.to(torch.float64), None, t, row8, 5, 250, bit_depth=12)
    for dtype in (torch.int16, torch.float64, torch.int32):
        with pytest.raises(TypeError, match="image_value_stack must be uint8 digital numbers"):
            e.linearity_energy(u8.to(dtype), None, t, row8, 5, 250)
    with pytest.raises(ValueError, match="4096"):
        e.linearity_energy(u16, None, t, row8, 5, 250, bit_depth=12)
    with pytest.raises(ValueError, match="256"):
        e.linearity_energy(u8, None, t, row12, 5, 250)
    for lower, upper in ((-1, 250), (5, 4096)):
        with pytest.raises(ValueError):
            e.linearity_energy(u16, None, t, row12, lower, upper, bit_depth=12)
    with pytest.raises(ValueError):
        e.linearity_energy(u16, None, t, row12, 5, 250, bit_depth=12, variant=3)
    assert e.linearity_energy(u16, None, t, row12, 0, 4095, bit_depth=12).shape == (1,)
    # the plans of the device solver keep refusing anything but uint8 stacks
    with pytest.raises(TypeError, match="image_value_stack must be uint8 digital numbers"):
        e.DEPlan(u16, None, t, row12[0], np.zeros((4096, 1)), [-1.0], [1.0], np.zeros((4, 1)), 5, 250, 1, 10, (0.0, 1.95), 0.4, 0.01, 0.0)
    # the calibration: SciPy's solver only
    mean, pca = np.linspace(0, 1, 4096) ** 2, np.zeros((4096, 1))
    for kw in (dict(solver="device"), dict(solver="device", restarts=2)):
        with pytest.raises(NotImplementedError, match='solver="scipy"'):
            ic.solve_channel(mean, pca, u16, None, t, -1.0, 1.0, bit_depth=12, **kw)
    for kw in (dict(solver="device"), dict(solver="device", batched=True), dict(solver="device", restarts=2)):
        with pytest.raises(NotImplementedError, match='solver="scipy"'):
            ic.calibration([mean], [pca], [u16], [None], t, -1.0, 1.0, bit_depth=12, **kw)
    with pytest.raises(ValueError, match="bit_depth"):
        ic.calibration([mean], [pca], [u16], [None], t, -1.0, 1.0, bit_depth=8)
    # the 8-bit messages are what they were
    with pytest.raises(ValueError, match='restarts > 1 needs solver="device"'):
        ic.solve_channel(mean[:256], pca[:256], u8, None, t, -1.0, 1.0, restarts=2)
    with pytest.raises(ValueError, match='batched=True needs solver="device"'):
        ic.calibration([mean[:256]], [pca[:256]], [u8], [None], t, -1.0, 1.0, batched=True)
    # frames
    f16 = [np.full((4, 4, 3), 4095, dtype=np.uint16) for _ in range(2)]
    with pytest.raises(ValueError, match="bit_depth"):
        ic.initialize_channel_image_stacks(f16, t, None, 1, device=dev)
    with pytest.raises(ValueError, match="bit_depth"):
        ic.initialize_channel_image_stacks([f.astype(np.uint8) for f in f16], t, None, 1, device=dev, bit_depth=12)
    stacks, _, _ = ic.initialize_channel_image_stacks(f16, t, None, 1, device=dev, bit_depth=12)
    assert len(stacks) == 3 and stacks[0].dtype == torch.uint16 and stacks[0].shape == (4, 4, 2) and int(stacks[0].cpu().numpy().max()) == 4095
    assert ic.interpolate_ICRF(np.linspace(0, 1, 256)[:, None] ** 2, bits=4096).shape == (4096, 1)
    assert ic.interpolate_ICRF(np.zeros((256, 1))).shape == (256, 1)
    # the power-law base takes its grid from the PCA basis
    assert ic.candidate_icrfs(np.array([2.0, 0.0]), None, pca, use_mean_ICRF=False)[0].shape == (1, 4096)


def test_python_surface():
    check_python_surface("cpu")


# ------------------------------------------------------------------------------------------------ 7: end to end at 12 bits
def check_calibration_12_bits(dev, iterations=40):
    """tests/test_gpu_producers.py::test_calibration_recovers_response on a 4096-point grid. In the NumPy oracle e0 / e_true = 455."""
    rng = np.random.default_rng(21)
    X, Y, N, n = 40, 40, 6, 4096
    t = 1e-3 * 2.0 ** np.arange(N)
    xs = np.linspace(0, 1, n)
    pca = np.stack([np.sin(np.pi * (m + 1) * xs) / (m + 1) for m in range(3)], axis=1) * 0.1
    mean_icrf = xs ** 2.0
    true_params = np.array([0.6, -0.3, 0.2])
    true_icrf, ok = ic.candidate_icrfs(true_params, mean_icrf, pca)
    assert ok[0] and true_icrf.shape == (1, n)
    rad = rng.random((X, Y)) * 2.5 / t[-1]
    lin = np.clip(rad[..., None] * t, 0, 1)
    dn = np.clip(np.around(np.interp(lin, true_icrf[0], xs) * (n - 1)), 0, n - 1).astype(np.uint16)
    frames = [dn[:, :, None, i].repeat(2, axis=2) for i in range(N)]
    stacks, stds, tt = ic.initialize_channel_image_stacks(frames, t, None, 1, device=dev, bit_depth=12)
    assert len(stacks) == 2 and stacks[0].shape == (X, Y, N) and np.array_equal(stacks[0].cpu().numpy(), dn)
    lower, upper = 5 << 4, 250 << 4
    e0 = ic._energy_function(np.zeros(3), mean_icrf, pca, stacks[0], None, lower, upper, True, tt, 12)
    e_true = ic._energy_function(true_params, mean_icrf, pca, stacks[0], None, lower, upper, True, tt, 12)
    print(f"e0 = {e0:.6g}, e_true = {e_true:.6g}, e0 / e_true = {e0 / e_true:.4g}")
    assert e_true < e0 / 10
    icrf, e, n_it = ic.solve_channel(mean_icrf, pca, stacks[0], None, tt, -1.0, 1.0, data_limits=(lower, upper), seed=7,
                                     max_iterations=iterations, vectorized=True, bit_depth=12)
    print(f"solve_channel: e = {e:.6g} after {n_it} iterations")
    assert icrf.shape == (n,) and n_it <= iterations
    assert e < e0 / 10, (e, e0, e_true)
    icrf1, e1, _ = ic.solve_channel(mean_icrf, pca, stacks[0], None, tt, -1.0, 1.0, data_limits=(lower, upper), seed=7, max_iterations=2,
                                    vectorized=False, bit_depth=12)
    assert icrf1.shape == (n,) and np.isfinite(e1)
    ICRF, energies = ic.calibration([mean_icrf] * 2, [pca] * 2, stacks, stds, tt, -1.0, 1.0, data_limits=(lower, upper), max_iterations=3,
                                    bit_depth=12)
    assert ICRF.shape == (n, 2) and energies.shape == (2,) and ICRF[0, 0] == 0 and ICRF[-1, 0] == 1
    out = eng(dev).merge([T(f, dev) for f in frames], t, ICRF, bit_depth=12)
    assert out["val"].shape == (X, Y, 2) and bool(torch.isfinite(out["val"]).any())


def test_calibration_at_12_bits():
    check_calibration_12_bits("cpu")
