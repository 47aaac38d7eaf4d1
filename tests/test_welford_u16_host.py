"""The Welford mean / std producer on the uint16 frames of 9- to 16-bit cameras (hm_welford_update_u16, hm_welford_finalize_u16,
engine.welford_update / welford_finalize(..., bit_depth=b), video_processing.welford_algorithm(..., bit_depth=b)) on the HOST build. The
checks are functions of a device name: tests/test_gpu_welford_u16.py runs the same ones on the MI355X.

Everything is compared bit for bit: the float64 state as int64 views, the uint16 frames with array_equal. With what:
    embedding   an 8-bit stack and ICRF embedded at depth b (DN << (b - 8), the 256 rows at k << (b - 8), every other row NaN) gives
                hm_welford_update's mean and m2; without an ICRF at 16 bits DN16 = 257 * DN8 does (257 k / 65535 = k / 255).
    oracle      oracle/hdr_oracle.py's welford_state (it indexes icrf[frame, arange(C)]: any depth). Without an ICRF the library gets
                icrf=None and the oracle the table arange(n) / M: NumPy's division is IEEE, which is the claim under test.
    finalize    np.around(mean * M).astype(uint16) and np.around(sqrt(m2 / (count - 1)) / sqrt(count)).astype(uint16), restated here (the
                oracle's are fixed at 255 / uint8), on states whose products lie in [0, 65535].
Every placement of the frame value that the rules allow for a call (variant 0, 1 = LDS where the table fits, 2 = computed without an ICRF,
3 = global memory with one) is exercised; the host build checks the variant and ignores it. The argument rules are called through ctypes
on both builds: every refusal returns before anything is launched, so the device library answers them on host pointers."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from camera_linearity_amd import video_processing as vp
from oracle import hdr_oracle as orc

# (H, W, C): only the odd tail; 189 elements, odd; even; C = 2; C = 4; 12 864 elements, several workgroups; 540 000 elements = 270 000
# lane pairs, more than one pass of the LDS form's grid (256 workgroups of 1024); 540 000 pairs, more than one pass of the 256-thread
# forms' grid (2048 workgroups)
SMALL_SHAPES = [(1, 1, 1), (7, 9, 3), (12, 20, 3), (5, 8, 2), (3, 5, 4), (64, 67, 3)]
LARGE_SHAPES = {(300, 600, 3): 3, (600, 600, 3): 2}                        # shape -> frames
SHAPES = SMALL_SHAPES + list(LARGE_SHAPES)
FRAME_COUNTS = [1, 7, 8, 9, 32, 45]                                         # 45: two launches, 32 + 13 (count_before)
DEPTHS = [9, 12, 13, 14, 16]
LDS, COMPUTED, GLOBAL = 1, 2, 3
LDS_TABLE_BYTES = 128 * 1024                                                # hm_producer_rules.h: kWelfordU16LdsTableBytes
TAB = {LDS: "lds", COMPUTED: "computed", GLOBAL: "global"}


def eng(dev):
    """engine on device tensors, the host build of the same functions on host tensors"""
    return engine if torch.device(dev).type == "cuda" else vp._engine_for(torch.device("cpu"))


def T(a, dev):
    """a fresh tensor on `dev` (never the array's own memory: the state is updated in place)"""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.clone() if torch.device(dev).type == "cpu" else t.to(dev)


def bits_of(t):
    return t.cpu().numpy().view(np.int64)


def fits_lds(depth, C, with_icrf):
    return 8 * 2 ** depth * (C if with_icrf else 1) <= LDS_TABLE_BYTES


def default_placement(depth, C, with_icrf):
    """hm_rules::welford_u16_default_placement"""
    if fits_lds(depth, C, with_icrf):
        return LDS
    return GLOBAL if with_icrf else COMPUTED


def variants(depth, C, with_icrf):
    """0 and every forced placement that exists for the call"""
    return [0] + ([LDS] if fits_lds(depth, C, with_icrf) else []) + ([GLOBAL] if with_icrf else [COMPUTED])


def kernel_of(n_elems, n_frames, Cc, with_icrf, with_m2, depth, variant, lib=None):
    """the DEVICE library's name of the kernel of such a call (hm_welford_update_u16_describe launches nothing: any machine)"""
    buf = C.create_string_buffer(128)
    rc = (lib or nat.hip_lib).hm_welford_update_u16_describe(n_elems, n_frames, Cc, int(with_icrf), int(with_m2), depth, variant, buf, len(buf))
    assert rc == nat.HM_OK, rc
    return buf.value.decode()


def fold(dev, frames_d, depth, table, variant=0, count0=0, mean0=None, m2_0=None, with_m2=True, per_launch=32):
    """frames_d: device frames. -> (mean, m2, count) after folding them `per_launch` at a time"""
    shape = tuple(frames_d[0].shape)
    mean = T(np.zeros(shape) if mean0 is None else mean0, dev)
    m2 = T(np.zeros(shape) if m2_0 is None else m2_0, dev) if with_m2 else None
    count = count0
    for k0 in range(0, len(frames_d), per_launch):
        count = eng(dev).welford_update(frames_d[k0:k0 + per_launch], count, mean, m2, table, bit_depth=depth, variant=variant)
    return mean, m2, count


def same_bits(got, want, what):
    assert np.array_equal(bits_of(got) if isinstance(got, torch.Tensor) else got.view(np.int64), want.view(np.int64)), what


def monotone_table(rng, n, C):
    """a random strictly increasing ICRF from 0 to 1 per channel"""
    t = np.cumsum(rng.random((n, C)) + 1e-3, axis=0)
    t = (t - t[0]) / (t[-1] - t[0])
    return np.ascontiguousarray(t)


def linear_table(depth, C):
    n = 2 ** depth
    return np.repeat((np.arange(n) / (n - 1))[:, None], C, axis=1)


# ------------------------------------------------------------------------------------------------ 1: embedding
def check_embedding(dev, shape, depth):
    H, W, Cc = shape
    rng = np.random.default_rng(1000 * H + depth)
    s = depth - 8
    for N in (9, 45):
        dn8 = rng.integers(0, 256, (N, H, W, Cc), dtype=np.uint8)
        icrf8 = np.linspace(0, 1, 256)[:, None] ** (1.5 + 0.3 * np.arange(Cc))[None, :]
        f8 = [T(f, dev) for f in dn8]
        ref_mean, ref_m2 = T(np.zeros(shape), dev), T(np.zeros(shape), dev)
        eng(dev).welford_update(f8, 0, ref_mean, ref_m2, icrf8)                              # hm_welford_update
        ref_mean, ref_m2 = ref_mean.cpu().numpy(), ref_m2.cpu().numpy()
        assert not np.isnan(ref_mean).any() and not np.isnan(ref_m2).any()
        wide = np.full((2 ** depth, Cc), np.nan)
        wide[np.arange(256) << s] = icrf8
        f16 = [T(f.astype(np.uint16) << s, dev) for f in dn8]
        for v in variants(depth, Cc, True):
            mean, m2, count = fold(dev, f16, depth, wide, v)
            assert count == N
            same_bits(mean, ref_mean, (shape, depth, N, v, "mean"))
            same_bits(m2, ref_m2, (shape, depth, N, v, "m2"))
        if depth == 16:                                                                      # no ICRF: 257 k / 65535 = k / 255
            m8, q8 = T(np.zeros(shape), dev), T(np.zeros(shape), dev)
            eng(dev).welford_update(f8, 0, m8, q8)
            assert not np.isnan(m8.cpu().numpy()).any() and not np.isnan(q8.cpu().numpy()).any()
            f257 = [T(f.astype(np.uint16) * 257, dev) for f in dn8]
            for v in variants(16, Cc, False):
                mean, m2, _ = fold(dev, f257, 16, None, v)
                same_bits(mean, m8.cpu().numpy(), (shape, N, v, "mean, no ICRF"))
                same_bits(m2, q8.cpu().numpy(), (shape, N, v, "m2, no ICRF"))


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_embedding_bit_patterns(shape, depth):
    check_embedding("cpu", shape, depth)


# ------------------------------------------------------------------------------------------------ 2: the oracle at full range
def check_oracle(dev, shape, depth, with_icrf):
    H, W, Cc = shape
    n = 2 ** depth
    rng = np.random.default_rng(7 * H + 31 * depth + with_icrf)
    table = monotone_table(rng, n, Cc) if with_icrf else None
    oracle_table = table if with_icrf else linear_table(depth, Cc)
    for N in ([LARGE_SHAPES[shape]] if shape in LARGE_SHAPES else FRAME_COUNTS):
        frames = rng.integers(0, n, (N, H, W, Cc)).astype(np.uint16)                         # uniform over 0..M
        ref_mean, ref_m2, cnt = orc.welford_state(list(frames), oracle_table, True)
        assert not np.isnan(ref_mean).any() and not np.isnan(ref_m2).any()
        fd = [T(f, dev) for f in frames]
        for v in variants(depth, Cc, with_icrf):
            mean, m2, count = fold(dev, fd, depth, table, v)
            assert count == cnt == N
            same_bits(mean, ref_mean, (shape, depth, N, v, "mean"))
            same_bits(m2, ref_m2, (shape, depth, N, v, "m2"))
        mean, m2, _ = fold(dev, fd, depth, table, 0, with_m2=False)                          # m2 is nullable
        assert m2 is None
        same_bits(mean, ref_mean, (shape, depth, N, "mean without m2"))


@pytest.mark.parametrize("with_icrf", [False, True])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_oracle(shape, depth, with_icrf):
    check_oracle("cpu", shape, depth, with_icrf)


def check_stray_high_bits(dev, depth):
    """DNs above M: the library masks before every table access; the oracle is fed DN & M"""
    shape, N = (12, 20, 3), 9
    n = 2 ** depth
    rng = np.random.default_rng(depth)
    frames = rng.integers(0, n, (N,) + shape).astype(np.uint16)
    stray = (frames | (rng.integers(0, 2 ** (16 - depth), frames.shape) << depth)).astype(np.uint16)
    assert (stray != frames).any() and np.array_equal(stray & (n - 1), frames)
    for with_icrf in (False, True):
        table = monotone_table(rng, n, 3) if with_icrf else None
        ref_mean, ref_m2, _ = orc.welford_state(list(frames), table if with_icrf else linear_table(depth, 3), True)
        assert not np.isnan(ref_mean).any() and not np.isnan(ref_m2).any()
        fd = [T(f, dev) for f in stray]
        for v in variants(depth, 3, with_icrf):
            mean, m2, _ = fold(dev, fd, depth, table, v)
            same_bits(mean, ref_mean, (depth, with_icrf, v))
            same_bits(m2, ref_m2, (depth, with_icrf, v))


@pytest.mark.parametrize("depth", [9, 12, 15])
def test_stray_high_bits_are_masked(depth):
    check_stray_high_bits("cpu", depth)


# ------------------------------------------------------------------------------------------------ 3: the computed quotient, exhaustively
def check_computed_quotient(dev, depth):
    """one frame holding every DN of 0..M, zero state, no ICRF, variant = computed: mean = f = DN / M with the IEEE division"""
    n = 2 ** depth
    frame = np.arange(n, dtype=np.uint16).reshape(1, n, 1)
    want = np.arange(n) / (n - 1)
    assert not np.isnan(want).any()
    for v in (COMPUTED, 0):
        mean, m2, _ = fold(dev, [T(frame, dev)], depth, None, v)
        same_bits(mean, want.reshape(1, n, 1), (depth, v))
        assert not m2.cpu().numpy().any()


@pytest.mark.parametrize("depth", range(9, 17))
def test_computed_quotient_is_the_ieee_quotient(depth):
    check_computed_quotient("cpu", depth)


# ------------------------------------------------------------------------------------------------ 4: the fast-division range
RANGE_CASES = ["signed_table", "tiny_entry", "tiny_state", "huge_state", "nan_state", "zero_runs"]


def check_fast_division_range(dev, case):
    """tests/test_gpu_producers.py::test_welford_fast_division_range at depth 12, in every placement"""
    depth, n = 12, 4096
    rng = np.random.default_rng(len(case))
    shape, N = (9, 14, 3), 41
    clip = rng.integers(0, n, (N,) + shape).astype(np.uint16)
    icrf = np.linspace(0, 1, n)[:, None] ** np.array([1.7, 2.0, 2.3])[None, :]
    mean0 = np.zeros(shape)
    tables = [True]
    if case == "signed_table":
        icrf = icrf - 0.37                                                 # both signs: m (1 - 1/n) + f/n cancels
        icrf[1600] = -icrf[1601]
    elif case == "tiny_entry":
        icrf[7, 1] = 1e-200                                                # outside [2^-500, 2^500]
        clip[3, 2, 2, 1] = 7                                               # ... and read
    elif case == "tiny_state":
        mean0[2, 3, 1] = 1e-250
        mean0[4, 5, 0] = -3e-300
        tables = [True, False]
    elif case == "huge_state":
        mean0[1, 1, 2] = 1e200
        tables = [True, False]
    elif case == "nan_state":
        mean0[0, 0, 0] = np.nan
        tables = [True, False]
    elif case == "zero_runs":
        clip[5:30] = 0                                                     # ICRF[0] = 0: twenty-five frames of f = 0
        icrf[0] = 0.0
        tables = [True, False]
    count0 = 3 if case.endswith("state") else 0
    fd = [T(f, dev) for f in clip]
    for with_icrf in tables:
        with np.errstate(all="ignore"):
            ref_mean, ref_m2, cnt = orc.welford_state(list(clip), icrf if with_icrf else linear_table(depth, 3), True, mean=mean0.copy(),
                                                      m2=np.zeros(shape), count=count0)
        assert case == "nan_state" or not (np.isnan(ref_mean).any() or np.isnan(ref_m2).any())
        if case == "nan_state":
            assert np.isnan(ref_mean).sum() == 1 and np.isnan(ref_mean[0, 0, 0])
        vs = variants(depth, 3, with_icrf)
        assert vs == ([0, LDS, GLOBAL] if with_icrf else [0, LDS, COMPUTED])
        for v in vs:
            mean, m2, count = fold(dev, fd, depth, icrf if with_icrf else None, v, count0=count0, mean0=mean0, per_launch=16)
            assert count == cnt
            np.testing.assert_array_equal(mean.cpu().numpy(), ref_mean, err_msg=str((case, with_icrf, v)))
            np.testing.assert_array_equal(m2.cpu().numpy(), ref_m2, err_msg=str((case, with_icrf, v)))
            keep = ~np.isnan(ref_mean)
            same_bits(mean.cpu().numpy()[keep], ref_mean[keep], (case, with_icrf, v))
            same_bits(m2.cpu().numpy()[keep], ref_m2[keep], (case, with_icrf, v))


@pytest.mark.parametrize("case", RANGE_CASES)
def test_fast_division_range(case):
    check_fast_division_range("cpu", case)


# ------------------------------------------------------------------------------------------------ 5: alignment and tails
def check_alignment(dev, shape, depth, with_icrf):
    """frames at 2-byte-aligned (not 4-byte-aligned) addresses, state at 8-byte-aligned (not 16-byte-aligned) ones: the aligned call's bits"""
    H, W, Cc = shape
    E, N, n = H * W * Cc, 9, 2 ** depth
    rng = np.random.default_rng(E + depth)
    frames = rng.integers(0, n, (N, E)).astype(np.uint16)
    table = monotone_table(rng, n, Cc) if with_icrf else None
    ref_mean, ref_m2, _ = orc.welford_state(list(frames.reshape((N,) + shape)), table if with_icrf else linear_table(depth, Cc), True)
    assert not np.isnan(ref_mean).any() and not np.isnan(ref_m2).any()
    pad = E + (E & 1) + 2                                                  # an even stride from an odd start: every frame at 2 (mod 4)
    buf = torch.zeros(N * pad + 1, dtype=torch.int16, device=dev)
    for k in range(N):
        buf[1 + k * pad: 1 + k * pad + E] = T(frames[k].view(np.int16), dev)
    off = [buf.view(torch.uint16)[1 + k * pad: 1 + k * pad + E].view(shape) for k in range(N)]
    assert all(f.data_ptr() % 4 == 2 and f.is_contiguous() for f in off)
    aligned = [T(f.reshape(shape), dev) for f in frames]
    for v in variants(depth, Cc, with_icrf):
        for fr, state_off in ((aligned, 0), (off, 0), (aligned, 1), (off, 1)):
            sm = torch.zeros(E + 2, dtype=torch.float64, device=dev)
            sq = torch.zeros(E + 2, dtype=torch.float64, device=dev)
            mean, m2 = sm[state_off:state_off + E].view(shape), sq[state_off:state_off + E].view(shape)
            if dev != "cpu":
                assert mean.data_ptr() % 16 == 8 * state_off
            eng(dev).welford_update(fr, 0, mean, m2, table, bit_depth=depth, variant=v)
            same_bits(mean, ref_mean, (shape, depth, v, state_off, "mean"))
            same_bits(m2, ref_m2, (shape, depth, v, state_off, "m2"))
            assert float(sm[E + 1 if state_off == 0 else 0]) == 0.0 and float(sq[E + 1 if state_off == 0 else 0]) == 0.0   # nothing beside the view


@pytest.mark.parametrize("with_icrf", [False, True])
@pytest.mark.parametrize("shape", [(7, 9, 3), (12, 20, 3), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_alignment_and_tails(shape, with_icrf):
    for depth in (12, 16):
        check_alignment("cpu", shape, depth, with_icrf)


# ------------------------------------------------------------------------------------------------ 6: finalize
def finalize_reference(mean, m2, count, depth):
    M = 2 ** depth - 1
    return np.around(mean * M).astype(np.uint16), np.around(np.sqrt(m2 / (count - 1)) / np.sqrt(count)).astype(np.uint16)


def check_finalize(dev, depth):
    M, count = 2 ** depth - 1, 4
    rng = np.random.default_rng(depth)
    ties = np.array([t for t in (0.5, 1.5, 2.5) if t * M <= 65535])                         # M is odd: t * M ends in .5 exactly
    mean = np.concatenate([rng.random(500), [0.0, 1.0, 65535 / M], ties])
    mean = mean[mean * M <= 65535]
    j = np.arange(0, 600, 7, dtype=np.float64)
    m2 = np.concatenate([3.0 * (2 * j + 1) ** 2, rng.random(mean.size) * 1e9])[:mean.size]   # sqrt(3 (2j + 1)^2 / 3) / 2 = j + 0.5: ties
    mean, m2 = mean.reshape(-1, 1, 1), m2.reshape(-1, 1, 1)
    assert ((mean * M) % 1 == 0.5).sum() >= ties.size and ((np.sqrt(m2 / 3) / 2) % 1 == 0.5).sum() >= 80
    assert (np.sqrt(m2 / 3) / 2).max() <= 65535 and not np.isnan(mean).any() and not np.isnan(m2).any()
    want_mean, want_std = finalize_reference(mean, m2, count, depth)
    got_mean, got_std = eng(dev).welford_finalize(T(mean, dev), T(m2, dev), count, bit_depth=depth)
    assert got_mean.dtype == torch.uint16 and got_std.dtype == torch.uint16 and got_mean.shape == mean.shape
    assert np.array_equal(got_mean.cpu().numpy(), want_mean) and np.array_equal(got_std.cpu().numpy(), want_std)
    only_mean, none = eng(dev).welford_finalize(T(mean, dev), None, 1, bit_depth=depth)
    assert none is None and np.array_equal(only_mean.cpu().numpy(), want_mean)
    # NaN gives 0 (NumPy's cast of it is not defined)
    nan_mean, nan_std = eng(dev).welford_finalize(T(np.full((3, 1, 1), np.nan), dev), T(np.array([np.nan, -1.0, 12.0]).reshape(3, 1, 1), dev), count,
                                                  bit_depth=depth)
    assert nan_mean.cpu().numpy().tolist() == [[[0]]] * 3 and nan_std.cpu().numpy().ravel().tolist() == [0, 0, 1]


def check_rounding_out_of_range(dev):
    """round_to_u16(x) & 255 == round_to_u8(x), through the std output (it is not rescaled: the same x in both entries); device == host"""
    x = np.array([65535.5, 65536.0, 65537.0, 1e5, 123456789.0, 2.0 ** 40 + 77, 1e18, 9.1e18, 9.3e18, 1e30, np.inf, 300.5, 255.5, 256.5, 70000.49])
    count = 4
    m2 = (3.0 * (2.0 * x) ** 2).reshape(-1, 1, 1)                                             # sqrt(m2 / 3) / 2 = x where that is exact
    m2 = np.concatenate([m2, np.array([np.nan, -4.0]).reshape(-1, 1, 1)])
    mean = np.zeros(m2.shape)
    _, s16 = eng(dev).welford_finalize(T(mean, dev), T(m2, dev), count, bit_depth=12)
    _, s8 = eng(dev).welford_finalize(T(mean, dev), T(m2, dev), count)
    _, h16 = eng("cpu").welford_finalize(T(mean, "cpu"), T(m2, "cpu"), count, bit_depth=12)
    s16, s8, h16 = s16.cpu().numpy(), s8.cpu().numpy(), h16.numpy()
    assert s8.dtype == np.uint8 and np.array_equal(s16 & 255, s8)
    assert np.array_equal(s16, h16)
    assert s16.ravel()[8:11].tolist() == [0, 0, 0] and s16.ravel()[-2:].tolist() == [0, 0]      # beyond 9.2e18, inf; NaN
    assert len(set(s16.ravel()[:8].tolist())) > 4                                               # the others are not all alike


@pytest.mark.parametrize("depth", DEPTHS)
def test_finalize(depth):
    check_finalize("cpu", depth)


def test_rounding_out_of_range():
    check_rounding_out_of_range("cpu")


# ------------------------------------------------------------------------------------------------ 7: the rules, both builds
EINVAL, ESHAPE, EUNSUP, EALIGN, OK = nat.HM_EINVAL, nat.HM_ESHAPE, nat.HM_EUNSUPPORTED, nat.HM_EALIGN, nat.HM_OK
_KEEP = dict(frame=np.full(16, 100, np.uint16), icrf=np.tile(np.linspace(0, 1, 65536)[:, None], (1, 4)).copy(), mean=np.zeros(12), m2=np.zeros(12),
             out_mean=np.zeros(16, np.uint16), out_std=np.zeros(16, np.uint16))
ICRF = _KEEP["icrf"].ctypes.data


def _update_call(lib, **over):
    """hm_welford_update_u16 on host buffers: 2 frames of 12 elements (C = 3) at 12 bits, no ICRF, with the faults of `over`; -> status.
    frames_at: {index: address} replaces entries of the frame array."""
    _KEEP["mean"][:] = 0
    _KEEP["m2"][:] = 0
    a = dict(frames=(C.c_void_p * 33)(*[_KEEP["frame"].ctypes.data] * 33), n_frames=2, count_before=0, icrf=None, mean=_KEEP["mean"].ctypes.data,
             m2=_KEEP["m2"].ctypes.data, n_elems=12, C=3, bit_depth=12, variant=0, stream=None)
    over = dict(over)
    for i, p in over.pop("frames_at", {}).items():
        a["frames"][i] = p
    a.update(over)
    return lib.hm_welford_update_u16(*a.values())


# (stage in the header's order, the change, its status); every fault alone, then every pair that pins the order
UPDATE_FAULTS = [
    (1, dict(n_frames=-1), EINVAL), (1, dict(n_frames=33), EINVAL), (1, dict(count_before=-1), EINVAL), (1, dict(n_elems=-1), EINVAL),
    (1, dict(bit_depth=8), EINVAL), (1, dict(bit_depth=17), EINVAL), (1, dict(variant=-1), EINVAL), (1, dict(variant=4), EINVAL),
    (2, dict(count_before=(1 << 40) + 1), EUNSUP),
    (3, dict(C=0), ESHAPE), (3, dict(C=5), ESHAPE), (4, dict(n_elems=11), ESHAPE),
    (5, dict(n_frames=0), OK), (5, dict(n_elems=0), OK),
    (6, dict(variant=GLOBAL), EUNSUP), (6, dict(variant=COMPUTED, icrf=ICRF), EUNSUP), (6, dict(variant=LDS, bit_depth=15), EUNSUP),
    (6, dict(variant=LDS, bit_depth=13, icrf=ICRF), EUNSUP),
    (7, dict(frames=None), EINVAL), (7, dict(mean=None), EINVAL), (7, dict(frames_at={0: None}), EINVAL), (7, dict(frames_at={1: None}), EINVAL),
    (8, dict(frames_at={1: _KEEP["frame"].ctypes.data + 1}), EALIGN),
]


def _libs():
    return [("device", nat.hip_lib), ("host", nat.host_lib())]


def _merged(o1, o2):
    out = {**o1, **o2}
    if "frames_at" in o1 and "frames_at" in o2:
        out["frames_at"] = {**o1["frames_at"], **o2["frames_at"]}
    return out


def test_update_rules_every_status_in_order():
    for name, lib in _libs():
        for stage, over, code in UPDATE_FAULTS:
            assert _update_call(lib, **over) == code, (name, over)
        for (s1, o1, c1), (s2, o2, c2) in itertools.permutations(UPDATE_FAULTS, 2):
            if s1 < s2 and c1 != c2 and not (set(o1) & set(o2)) - {"frames_at"}:
                if "frames" in o1 and "frames_at" in o2 or o1.get("frames_at", {}).keys() & o2.get("frames_at", {}).keys():
                    continue
                assert _update_call(lib, **_merged(o1, o2)) == c1, (name, o1, o2)
    host = nat.host_lib()
    # what is allowed: the limits of every rule, and every placement where it applies (the host build runs these)
    assert _update_call(host) == OK and _KEEP["mean"][0] == 100 / 4095 and _KEEP["m2"][0] == 0.0
    for over in (dict(count_before=1 << 40), dict(n_frames=32), dict(bit_depth=9), dict(bit_depth=16), dict(m2=None), dict(variant=LDS),
                 dict(variant=COMPUTED), dict(variant=LDS, bit_depth=14), dict(variant=COMPUTED, bit_depth=16), dict(variant=GLOBAL, icrf=ICRF),
                 dict(variant=LDS, icrf=ICRF), dict(variant=GLOBAL, icrf=ICRF, bit_depth=16), dict(variant=LDS, icrf=ICRF, bit_depth=14, C=1),
                 dict(variant=LDS, icrf=ICRF, bit_depth=13, C=2, n_elems=12), dict(variant=LDS, icrf=ICRF, bit_depth=12, C=4)):
        assert _update_call(host, **over) == OK, over
    for over in (dict(variant=LDS, icrf=ICRF, bit_depth=15, C=1), dict(variant=LDS, icrf=ICRF, bit_depth=14, C=2), dict(variant=LDS, icrf=ICRF, bit_depth=13, C=4)):
        for name, lib in _libs():
            assert _update_call(lib, **over) == EUNSUP, (name, over)
    # nothing to do: no pointer is looked at
    for name, lib in _libs():
        assert _update_call(lib, n_frames=0, frames=None, mean=None, m2=None) == OK, name
        assert _update_call(lib, n_elems=0, frames=None, mean=None, m2=None, variant=GLOBAL) == OK, name


def _finalize_call(lib, **over):
    a = dict(mean=_KEEP["mean"].ctypes.data, m2=_KEEP["m2"].ctypes.data, count=2, bit_depth=12, out_mean=_KEEP["out_mean"].ctypes.data,
             out_std=_KEEP["out_std"].ctypes.data, n_elems=12, stream=None)
    a.update(over)
    return lib.hm_welford_finalize_u16(*a.values())


FINALIZE_FAULTS = [
    (1, dict(n_elems=-1), EINVAL), (1, dict(count=0), EINVAL), (1, dict(count=-1), EINVAL), (1, dict(bit_depth=8), EINVAL), (1, dict(bit_depth=17), EINVAL),
    (2, dict(n_elems=0), OK),
    (3, dict(mean=None), EINVAL), (3, dict(m2=None), EINVAL), (4, dict(count=1), EINVAL),
    (5, dict(out_mean=_KEEP["out_mean"].ctypes.data + 1), EALIGN), (5, dict(out_std=_KEEP["out_std"].ctypes.data + 1), EALIGN),
]


def test_finalize_rules_every_status_in_order():
    for name, lib in _libs():
        for stage, over, code in FINALIZE_FAULTS:
            assert _finalize_call(lib, **over) == code, (name, over)
        for (s1, o1, c1), (s2, o2, c2) in itertools.permutations(FINALIZE_FAULTS, 2):
            if s1 < s2 and c1 != c2 and not set(o1) & set(o2):
                assert _finalize_call(lib, **_merged(o1, o2)) == c1, (name, o1, o2)
    host = nat.host_lib()
    assert _finalize_call(host) == OK
    assert _finalize_call(host, out_std=None, m2=None, count=1) == OK and _finalize_call(host, out_mean=None, mean=None) == OK
    for name, lib in _libs():
        assert _finalize_call(lib, n_elems=0, mean=None, m2=None, out_mean=None, out_std=None) == OK, name


def test_symbols_version_and_byte_count():
    for name, lib in _libs():
        for sym in ("hm_welford_update_u16", "hm_welford_finalize_u16", "hm_welford_u16_algorithmic_bytes", "hm_welford_update_u16_describe"):
            assert sym in nat.EXPORTED_SYMBOLS and callable(getattr(lib, sym)), (name, sym)
        assert lib.hm_version() == 2
        assert lib.hm_welford_u16_algorithmic_bytes(32, 1, 1000) == 1000 * (64 + 32)
        assert lib.hm_welford_u16_algorithmic_bytes(5, 0, 7) == 7 * (10 + 16)


def test_describe_names_the_placement_at_every_edge_of_the_fit_rule():
    n = 540000
    # (C, with an ICRF, depth) -> the library's choice; on each side of every edge of the fit rule
    expect = {(3, True, 12): "lds", (3, True, 13): "global", (4, True, 12): "lds", (4, True, 13): "global", (2, True, 13): "lds", (2, True, 14): "global",
              (1, True, 14): "lds", (1, True, 15): "global", (3, False, 14): "lds", (3, False, 15): "computed", (1, False, 14): "lds",
              (1, False, 15): "computed", (3, False, 16): "computed", (3, True, 16): "global", (3, True, 9): "lds", (3, False, 9): "lds"}
    for (Cc, with_icrf, depth), tab in expect.items():
        assert TAB[default_placement(depth, Cc, with_icrf)] == tab
        for with_m2 in (0, 1):
            assert kernel_of(n - n % Cc, 32, Cc, with_icrf, with_m2, depth, 0) == f"k_welford_u16<m2={with_m2},tab={tab},bits={depth}>"
        for v in (LDS, COMPUTED, GLOBAL):
            buf = C.create_string_buffer(64)
            applies = v in variants(depth, Cc, with_icrf)
            for name, lib in _libs():
                rc = lib.hm_welford_update_u16_describe(n - n % Cc, 32, Cc, int(with_icrf), 1, depth, v, buf, len(buf))
                assert rc == (OK if applies else EUNSUP), (name, Cc, with_icrf, depth, v)
                assert not applies or name == "host" or buf.value.decode() == f"k_welford_u16<m2=1,tab={TAB[v]},bits={depth}>"
    for name, lib in _libs():
        buf = C.create_string_buffer(64)
        assert lib.hm_welford_update_u16_describe(12, 2, 3, 0, 1, 12, 0, None, 0) == EINVAL, name
        assert lib.hm_welford_update_u16_describe(12, 2, 3, 0, 1, 8, 0, buf, len(buf)) == EINVAL, name
        assert lib.hm_welford_update_u16_describe(11, 2, 3, 0, 1, 12, 0, buf, len(buf)) == ESHAPE, name
        assert lib.hm_welford_update_u16_describe(12, 0, 3, 0, 1, 12, 0, buf, len(buf)) == OK and buf.value == b"", name
        assert lib.hm_welford_update_u16_describe(12, 2, 3, 0, 1, 12, 0, buf, len(buf)) == OK and buf.value, name
    assert engine.welford_kernel(12, 2, 3, True, True, 12, GLOBAL) == "k_welford_u16<m2=1,tab=global,bits=12>"
    with pytest.raises(NotImplementedError):
        engine.welford_kernel(12, 2, 3, True, True, 12, COMPUTED)


# ------------------------------------------------------------------------------------------------ 8: the Python surface
def check_python(dev):
    depth, n, shape, N = 12, 4096, (20, 30, 3), 45
    rng = np.random.default_rng(45)
    frames = rng.integers(0, n, (N,) + shape).astype(np.uint16)
    icrf = monotone_table(rng, n, 3)
    ref_mean, ref_m2, cnt = orc.welford_state(list(frames), icrf, True)
    assert not np.isnan(ref_mean).any() and not np.isnan(ref_m2).any()
    want_mean, want_std = finalize_reference(ref_mean, ref_m2, cnt, depth)
    assert want_mean.max() > 255                                             # a uint8 result could not hold it
    ret = vp.welford_algorithm(iter(frames), icrf, use_std=True, device=dev, bit_depth=depth)
    assert ret["mean"].dtype == np.uint16 and ret["std"].dtype == np.uint16
    assert np.array_equal(ret["mean"], want_mean) and np.array_equal(ret["std"], want_std)
    two = vp.welford_algorithm([list(frames[:20]), iter(frames[20:])], icrf, use_std=True, device=dev, bit_depth=depth, frames_per_launch=7)
    assert np.array_equal(two["mean"], want_mean) and np.array_equal(two["std"], want_std)
    tens = vp.welford_algorithm([T(f, dev) for f in frames], None, False, device=dev, bit_depth=depth, as_numpy=False)       # tensors, no ICRF
    lin_mean, _, _ = orc.welford_state(list(frames), linear_table(depth, 3), False)
    assert tens["std"] is None and tens["mean"].dtype == torch.uint16
    assert np.array_equal(tens["mean"].cpu().numpy(), np.around(lin_mean * (n - 1)).astype(np.uint16))
    # what is refused
    with pytest.raises((TypeError, ValueError), match="bit_depth"):
        vp.welford_algorithm(iter(frames), icrf, use_std=True, device=dev)                                # uint16 frames without a depth
    with pytest.raises(ValueError, match="bit_depth"):
        vp.welford_algorithm([f.astype(np.uint8) for f in frames[:3]], None, False, device=dev, bit_depth=depth)
    for bad in (8, 17, 12.0, True):
        with pytest.raises(ValueError, match="bit_depth"):
            vp.welford_algorithm(iter(frames), icrf, device=dev, bit_depth=bad)
    with pytest.raises(ValueError, match="4096"):
        vp.welford_algorithm(iter(frames), icrf[:256], device=dev, bit_depth=depth)                       # an ICRF of the wrong row count
    with pytest.raises(ValueError, match="256"):
        vp.welford_algorithm([f.astype(np.uint8) for f in frames[:3]], icrf, device=dev)
    with pytest.raises(ValueError, match="two frames"):
        vp.welford_algorithm(iter(frames[:1]), icrf, use_std=True, device=dev, bit_depth=depth)
    with pytest.raises((TypeError, ValueError)):
        vp.compute_noise_profiles([list(frames[:3])], device=dev)                                         # the noise profiles stay 8-bit
    with pytest.raises((TypeError, ValueError)):
        vp.compute_noise_profiles([list(frames[:3])], mean_frame=frames[0], device=dev)
    # the engine's two functions
    e = eng(dev)
    mean, fd = T(np.zeros(shape), dev), [T(f, dev) for f in frames[:3]]
    with pytest.raises(ValueError, match="bit_depth"):
        e.welford_update(fd, 0, mean, None)
    with pytest.raises(ValueError, match="bit_depth"):
        e.welford_update([f.to(torch.uint8) for f in fd], 0, mean, None, bit_depth=depth)
    with pytest.raises(ValueError, match="uint16"):
        e.welford_update(fd[:1] + [fd[1].to(torch.uint8)], 0, mean, None, bit_depth=depth)
    with pytest.raises(ValueError):
        e.welford_update(fd, 0, mean, None, bit_depth=depth, variant=4)
    with pytest.raises(NotImplementedError):
        e.welford_update(fd, 0, mean, None, bit_depth=depth, variant=GLOBAL)                              # no ICRF to gather from
    with pytest.raises(NotImplementedError):
        e.welford_update(fd, 0, mean, None, icrf, bit_depth=depth, variant=COMPUTED)
    assert not mean.cpu().numpy().any()                                                                   # a refused call changes nothing
    assert e.welford_update(fd, 0, mean, None, icrf, bit_depth=depth) == 3
    out_mean, out_std = e.welford_finalize(mean, None, 3)                                                 # bit_depth=None: the 8-bit result
    assert out_mean.dtype == torch.uint8 and out_std is None


def test_python_surface():
    check_python("cpu")


def test_save_result_writes_uint16_tiffs(tmp_path):
    from camera_linearity_amd import tiff_io
    frames = np.random.default_rng(2).integers(0, 4096, (4, 6, 8, 3)).astype(np.uint16)
    ret = vp.welford_algorithm(list(frames), None, True, device="cpu", bit_depth=12)
    vp.save_result(ret, tmp_path / "clip.avi")
    back = tiff_io.imread(tmp_path / "clip.mean.tif", tiff_io.IMREAD_UNCHANGED)
    assert back.dtype == np.uint16 and back.shape == (6, 8, 3)
