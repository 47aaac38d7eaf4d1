"""The per-DN STD table of 9- to 16-bit cameras from per-level noise moments (hm_noise_moments_update_u16, hm_noise_moments_std,
engine.noise_moments_update / noise_moments_std, video_processing.compute_noise_moments / noise_moments_to_STD_data) on the HOST build. The
checks are functions of a device name: tests/test_gpu_noise_moments.py runs the same ones on the MI355X.

With what:
    golden      tests/golden/noise.npz, the reference's own run on 8-bit clips. Widened to uint16 at bit_depth 9 the moments of levels 0..255
                are those of the golden profiles P[m, f, c] - sum_f P, sum_f (f - m) P, sum_f (f - m)^2 P - integer for integer, and the
                table * 511 / 255 is the golden std to assert_std_equal's rtol of 1e-13 (tests/test_noise_profiles_host.py).
    add.at      an np.add.at restatement of the three sums on masked DNs: integers, compared with array_equal.
    exact       the table against N = n S2 - S1^2 as a Python int and `decimal` at 80 digits, rounded once. Bound 8 * 2^-53 relative, derived:
                the value is at most five FP64 roundings from an exact numerator (two in the 128-bit conversion, the square root - which
                halves what it is given - and two divisions), 4 to 5 * 2^-53; the factor over that leaves the host compiler its
                contraction choices.
The argument rules are called through ctypes on both builds: every refusal returns before anything is launched, so the device library
answers them on host pointers."""
import ctypes as C
import decimal
import itertools
import math

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from camera_linearity_amd import video_processing as vp

DEPTHS = [9, 10, 11, 12, 16]
FRAME_COUNTS = [1, 2, 31, 32]
LDS, GLOBAL, WINDOW = 1, 2, 3
TAB = {LDS: "lds", GLOBAL: "global", WINDOW: "window"}
LDS_TABLE_BYTES, LDS_ENTRY_BYTES = 128 * 1024, 20      # hdrmerge.h: the LDS table, 20 * 2^bit_depth * C bytes, may take 128 KiB
STD_BOUND = 8 * 2.0 ** -53


def eng(dev):
    """engine on device tensors, the host build of the same functions on host tensors"""
    return engine if torch.device(dev).type == "cuda" else vp._engine_for(torch.device("cpu"))


def T(a, dev):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.clone() if torch.device(dev).type == "cpu" else t.to(dev)


def fits_lds(depth, Cc):
    return LDS_ENTRY_BYTES * 2 ** depth * Cc <= LDS_TABLE_BYTES


def variants(depth, Cc):
    """0 and every forced placement that exists for the call"""
    return [0] + ([LDS] if fits_lds(depth, Cc) else []) + [GLOBAL, WINDOW]


def add_at_moments(frames, mean, depth):
    """moments[m, c] += (1, d, d^2) for every frame and element, on masked DNs: the definition, with np.add.at"""
    M = 2 ** depth - 1
    Cc = mean.shape[-1]
    out = np.zeros((2 ** depth, Cc, 3), dtype=np.int64)
    m = (mean.astype(np.int64) & M).reshape(-1, Cc)
    c = np.broadcast_to(np.arange(Cc), m.shape)
    for f in frames:
        d = (f.astype(np.int64) & M).reshape(-1, Cc) - m
        np.add.at(out[:, :, 0], (m, c), 1)
        np.add.at(out[:, :, 1], (m, c), d)
        np.add.at(out[:, :, 2], (m, c), d * d)
    return out


def run_update(dev, frames_d, mean_d, depth, variant=0, into=None):
    mom = torch.zeros((2 ** depth, mean_d.shape[-1], 3), dtype=torch.int64, device=mean_d.device) if into is None else into
    eng(dev).noise_moments_update(frames_d, mean_d, mom, depth, variant)
    return mom


def offset_views(arrs, dev):
    """every array as a contiguous uint16 view that starts 2 bytes into a buffer (4-byte aligned + 2: no 16-byte loads on the device)"""
    out = []
    for a in arrs:
        buf = torch.zeros(a.size + 8, dtype=torch.int16, device=dev)
        buf[1:1 + a.size] = T(a.reshape(-1).view(np.int16), dev)
        v = buf.view(torch.uint16)[1:1 + a.size].view(a.shape)
        assert v.data_ptr() % 4 == 2 and v.is_contiguous()
        out.append(v)
    return out


# ------------------------------------------------------------------------------------------------ 1: the moments
def moment_case(hw, Cc, depth, N):
    """-> (frames, mean, stray frames, stray mean): noisy frames around a base image with d = +-M planted, and the same with bits set above
    the depth (the library masks them off; at 16 bits there are none)"""
    shape = hw + (Cc,)
    n, M = 2 ** depth, 2 ** depth - 1
    rng = np.random.default_rng(1000 * Cc + 10 * depth + N)
    base = rng.integers(0, n, shape)
    frames = np.clip(base + np.around(rng.standard_normal((N,) + shape) * max(2, n // 64)), 0, M).astype(np.uint16)
    mean = np.clip(base + rng.integers(-2, 3, shape), 0, M).astype(np.uint16)
    frames[0].reshape(-1)[:5] = [0, M, 0, M, M]
    mean.reshape(-1)[:5] = [M, 0, 0, M, 1]
    high = 2 ** (16 - depth)
    stray_f = (frames | (rng.integers(0, high, frames.shape) << depth)).astype(np.uint16)
    stray_m = (mean | (rng.integers(0, high, mean.shape) << depth)).astype(np.uint16)
    assert depth == 16 or ((stray_f != frames).any() and (stray_m != mean).any())
    return frames, mean, stray_f, stray_m


def check_moments(dev, hw, Cc, depth, reference):
    """every frame count, aligned and 2-byte-offset frames, stray high bits, a constant mean frame and two launches into one state, in every
    placement; reference(frames, mean, depth) -> the moments they must equal"""
    for N in FRAME_COUNTS:
        frames, mean, stray_f, stray_m = moment_case(hw, Cc, depth, N)
        want = reference(list(frames), mean, depth)
        assert want[:, :, 0].sum() == N * mean.size and (want[:, :, 2] >= np.abs(want[:, :, 1])).all()
        const = np.full_like(mean, int(mean.reshape(-1)[7]))
        want_const = reference(list(frames), const, depth)
        assert np.count_nonzero(want_const[:, :, 0]) == Cc
        inputs = {"aligned": ([T(f, dev) for f in stray_f], T(stray_m, dev)),
                  "offset": (offset_views(list(stray_f), dev), offset_views([stray_m], dev)[0])}
        for v in variants(depth, Cc):
            for kind, (fd, md) in inputs.items():
                got = run_update(dev, fd, md, depth, v).cpu().numpy()
                assert np.array_equal(got, want), (Cc, depth, N, v, kind)
            got = run_update(dev, inputs["aligned"][0], T(const, dev), depth, v).cpu().numpy()
            assert np.array_equal(got, want_const), (Cc, depth, N, v, "constant mean")
    # two launches into one state: the last case's 32 frames, then its first 31 again
    fd, md = inputs["aligned"]
    for v in variants(depth, Cc):
        mom = run_update(dev, fd, md, depth, v)
        run_update(dev, fd[:31], md, depth, v, into=mom)
        assert np.array_equal(mom.cpu().numpy(), want + reference(list(frames[:31]), mean, depth)), (Cc, depth, v, "two launches")


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
def test_moments_match_add_at(Cc, depth):
    check_moments("cpu", (7, 13), Cc, depth, add_at_moments)


# ------------------------------------------------------------------------------------------------ 2: the golden run of the reference
def golden_moments(profiles):
    """the moments of a (256, 256, C) noise profile P[m, f, c]: sum_f P, sum_f (f - m) P, sum_f (f - m)^2 P"""
    d = np.arange(256)[None, :] - np.arange(256)[:, None]
    return np.stack([profiles.sum(axis=1), (profiles * d[:, :, None]).sum(axis=1), (profiles * (d * d)[:, :, None]).sum(axis=1)], axis=2)


def check_golden(dev, z):
    from test_noise_profiles_host import assert_std_equal
    clips = [[f.astype(np.uint16) for f in z["clip_a"]], [f.astype(np.uint16) for f in z["clip_b"]]]
    mom, mean = vp.compute_noise_moments(clips, mean_frame=z["mean"].astype(np.uint16), device=dev, bit_depth=9)
    assert mom.dtype == np.int64 and mom.shape == (512, 3, 3) and mean.dtype == np.uint16 and np.array_equal(mean, z["mean"])
    assert np.array_equal(mom[:256], golden_moments(z["profiles"]))
    assert not mom[256:].any()
    table = vp.noise_moments_to_STD_data(mom, 9, device=dev)
    assert table.dtype == np.float64 and table.shape == (512, 3)
    assert_std_equal(table[:256] * 511 / 255, z["std"])
    assert np.isnan(table[256:]).all()
    # the default mean frame is welford_algorithm's at this depth: DN / 511 averaged, not the 8-bit run's DN / 255
    mom2, mean2 = vp.compute_noise_moments(clips, device=dev, bit_depth=9, frames_per_launch=7)
    want_mean = vp.welford_algorithm([clips[0], clips[1]], None, False, device=dev, bit_depth=9)["mean"]
    assert np.array_equal(mean2, want_mean)
    assert np.array_equal(mom2, add_at_moments(clips[0] + clips[1], want_mean, 9))


def test_golden_profiles_and_std(golden):
    check_golden("cpu", golden("noise"))


# ------------------------------------------------------------------------------------------------ 3: the table against an exact oracle
def exact_std(n, s1, s2, M):
    """sqrt(n S2 - S1^2) / n / M from the integer numerator at 80 digits, rounded once"""
    if n == 0:
        return math.nan
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        return float(decimal.Decimal(n * s2 - s1 * s1).sqrt() / n / M)


def table_cases(depth):
    """(n, S1, S2) triples as Python ints: sums of real d lists, so that n S2 >= S1^2 holds as it must"""
    M = 2 ** depth - 1
    rng = np.random.default_rng(depth)
    cases = [(0, 0, 0),                                                       # n = 0: NaN
             (5, 15, 45), (1, -M, M * M), (2 ** 40, 2 ** 40, 2 ** 40), (7, 0, 0)]   # N = 0: +0.0 (every d equal)
    far = 300 + rng.integers(-1, 2, 1000)                                     # a mean frame far from the true mean: |S1| large against S2
    cases.append((1000, int(far.sum()), int((far * far).sum())))
    cases.append((1000, -int(far.sum()), int((far * far).sum())))
    cases += [(2, 0, 2 * M * M), (3, M, 3 * M * M), (3, -M, 3 * M * M), (2 ** 20, 0, 2 ** 20 * M * M)]      # d = +-M
    # counts of 2^40: half the elements at d = a, half at d = b; then a quarter / three quarters
    for a, b in ((1, -1), (3, 2), (-181, 181), (100, -7)):
        h = 2 ** 39
        cases.append((2 ** 40, h * (a + b), h * (a * a + b * b)))
        cases.append((2 ** 40, h // 2 * (a + 3 * b), h // 2 * (a * a + 3 * b * b)))
    for _ in range(40):                                                       # noise of every width
        k = int(rng.integers(1, 2000))
        d = np.around(rng.standard_normal(k) * rng.choice([0.5, 3.0, 40.0, M / 8])).astype(np.int64).clip(-M, M)
        cases.append((k, int(d.sum()), int((d * d).sum())))
    assert all(0 <= n * s2 - s1 * s1 and s2 < 2 ** 63 and abs(s1) < 2 ** 63 for n, s1, s2 in cases)
    return cases


def check_table(dev, depth, Cc):
    cases = table_cases(depth)
    M, rows = 2 ** depth - 1, 2 ** depth
    mom = np.zeros((rows, Cc, 3), dtype=np.int64)
    want = np.full((rows, Cc), np.nan)
    slots = np.random.default_rng(depth + Cc).permutation(rows * Cc)[:len(cases)]
    for slot, (n, s1, s2) in zip(slots, cases):
        mom[slot // Cc, slot % Cc] = (n, s1, s2)
        want[slot // Cc, slot % Cc] = exact_std(n, s1, s2, M)
    got = vp.noise_moments_to_STD_data(mom, depth, device=dev)
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert ok.sum() == len(cases) - 1
    worst = np.max(np.abs(got[ok] - want[ok]) / np.where(want[ok] == 0, 1.0, want[ok]))
    print(f"noise_moments_std, {dev}, {depth} bits: worst relative distance from the exact table {worst / 2.0 ** -53:.3f} * 2^-53")
    assert (np.abs(got[ok] - want[ok]) <= STD_BOUND * want[ok]).all()
    zero = want == 0
    assert zero.sum() >= 4 and (got[zero] == 0).all() and not np.signbit(got[zero]).any()
    t = T(mom, dev)                                                           # a tensor stays a tensor on its device
    back = vp.noise_moments_to_STD_data(t, depth)
    assert isinstance(back, torch.Tensor) and back.device == t.device and np.array_equal(back.cpu().numpy(), got, equal_nan=True)


@pytest.mark.parametrize("depth,Cc", [(9, 1), (12, 3), (16, 3), (16, 4)])
def test_table_against_exact_oracle(depth, Cc):
    check_table("cpu", depth, Cc)


# ------------------------------------------------------------------------------------------------ 4: the rules, both builds
EINVAL, ESHAPE, EUNSUP, EALIGN, OK = nat.HM_EINVAL, nat.HM_ESHAPE, nat.HM_EUNSUPPORTED, nat.HM_EALIGN, nat.HM_OK
_KEEP = dict(frame=np.full(16, 100, np.uint16), mean=np.full(16, 98, np.uint16), mom=np.zeros((65536, 4, 3), np.int64), out=np.zeros((65536, 4)))


def _libs():
    return [("device", nat.hip_lib), ("host", nat.host_lib())]


def _update_call(lib, **over):
    """hm_noise_moments_update_u16 on host buffers: 2 frames of 12 elements (C = 3) at 11 bits, with the faults of `over`; -> status.
    frames_at: {index: address} replaces entries of the frame array."""
    _KEEP["mom"][:] = 0
    a = dict(frames=(C.c_void_p * 33)(*[_KEEP["frame"].ctypes.data] * 33), n_frames=2, mean=_KEEP["mean"].ctypes.data, n_elems=12, C=3, bit_depth=11,
             moments=_KEEP["mom"].ctypes.data, variant=0, stream=None)
    over = dict(over)
    for i, p in over.pop("frames_at", {}).items():
        a["frames"][i] = p
    a.update(over)
    return lib.hm_noise_moments_update_u16(*a.values())


# (stage in the header's order, the change, its status); every fault alone, then every pair that pins the order
UPDATE_FAULTS = [
    (1, dict(n_frames=-1), EINVAL), (1, dict(n_frames=33), EINVAL), (1, dict(n_elems=-1), EINVAL), (1, dict(C=0), EINVAL),
    (1, dict(bit_depth=8), EINVAL), (1, dict(bit_depth=17), EINVAL), (1, dict(variant=-1), EINVAL), (1, dict(variant=4), EINVAL),
    (2, dict(C=5), EUNSUP),
    (3, dict(n_elems=11), ESHAPE),
    (4, dict(variant=LDS, bit_depth=12), EUNSUP),
    (5, dict(frames=None), EINVAL), (5, dict(mean=None), EINVAL), (5, dict(moments=None), EINVAL), (5, dict(frames_at={0: None}), EINVAL),
    (5, dict(frames_at={1: None}), EINVAL),
    (6, dict(frames_at={1: _KEEP["frame"].ctypes.data + 1}), EALIGN), (6, dict(mean=_KEEP["mean"].ctypes.data + 1), EALIGN),
    (7, dict(n_frames=0), OK), (7, dict(n_elems=0), OK),
]


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
                if "frames_at" in o1 and "n_frames" in o2:                   # no frames: no frame pointer is looked at
                    continue
                assert _update_call(lib, **_merged(o1, o2)) == c1, (name, o1, o2)
        assert not _KEEP["mom"].any(), name                                  # a refused call changes nothing
    host = nat.host_lib()
    # what is allowed: the limits of every rule, and every placement where it fits (the host build runs these)
    assert _update_call(host) == OK
    assert _KEEP["mom"].reshape(-1)[98 * 9:99 * 9].tolist() == [8, 16, 32] * 3 and _KEEP["mom"].sum() == 3 * 56      # (2048, 3, 3), level 98
    for over in (dict(n_frames=32), dict(bit_depth=9), dict(bit_depth=16), dict(variant=LDS), dict(variant=GLOBAL), dict(variant=GLOBAL, bit_depth=16), dict(variant=WINDOW), dict(variant=WINDOW, bit_depth=16),
                 dict(variant=LDS, bit_depth=12, C=1), dict(variant=LDS, bit_depth=11, C=2), dict(variant=LDS, bit_depth=10, C=4)):
        assert _update_call(host, **over) == OK, over
    for over in (dict(variant=LDS, bit_depth=13, C=1), dict(variant=LDS, bit_depth=12, C=2), dict(variant=LDS, bit_depth=12, C=3),
                 dict(variant=LDS, bit_depth=11, C=4), dict(variant=LDS, bit_depth=16, C=1)):
        for name, lib in _libs():
            assert _update_call(lib, **over) == EUNSUP, (name, over)
            assert not _KEEP["mom"].any()
    for name, lib in _libs():                                                # nothing to do
        assert _update_call(lib, n_frames=0) == OK and _update_call(lib, n_elems=0) == OK and not _KEEP["mom"].any(), name


def test_std_rules():
    mom, out = _KEEP["mom"].ctypes.data, _KEEP["out"].ctypes.data
    for name, lib in _libs():
        for args in ((None, 3, 12, out), (mom, 3, 12, None), (mom, 0, 12, out), (mom, 3, 8, out), (mom, 3, 17, out), (None, 5, 12, out)):
            assert lib.hm_noise_moments_std(*args, None) == EINVAL, (name, args)
        assert lib.hm_noise_moments_std(mom, 5, 12, out, None) == EUNSUP, name
    _KEEP["mom"][:] = 0
    assert nat.host_lib().hm_noise_moments_std(mom, 4, 16, out, None) == OK and np.isnan(_KEEP["out"]).all()


def test_symbols_version_and_byte_count():
    for name, lib in _libs():
        for sym in ("hm_noise_moments_algorithmic_bytes", "hm_noise_moments_update_u16", "hm_noise_moments_update_u16_describe",
                    "hm_noise_moments_std"):
            assert sym in nat.EXPORTED_SYMBOLS and callable(getattr(lib, sym)), (name, sym)
        assert lib.hm_version() == 2
        assert lib.hm_noise_moments_algorithmic_bytes(32, 1000, 4, 16) == 2 * 1000 * 33 + 2 * 24 * 65536 * 4
        assert lib.hm_noise_moments_algorithmic_bytes(5, 9, 3, 10) == 2 * 9 * 6 + 2 * 24 * 1024 * 3


def describe(lib, n_elems, n_frames, Cc, depth, variant):
    buf = C.create_string_buffer(128)
    return lib.hm_noise_moments_update_u16_describe(n_elems, n_frames, Cc, depth, variant, buf, len(buf)), buf.value.decode()


def test_describe_names_the_placement_at_every_edge_of_the_fit_rule():
    # (C, depth) -> the library's choice, on each side of every edge of the fit rule
    expect = {(1, 12): "lds", (1, 13): "window", (2, 11): "lds", (2, 12): "window", (3, 11): "lds", (3, 12): "window", (4, 10): "lds",
              (4, 11): "window", (3, 9): "lds", (1, 9): "lds", (1, 16): "window", (3, 16): "window", (4, 16): "window"}
    for (Cc, depth), tab in expect.items():
        assert ("lds" if fits_lds(depth, Cc) else "window") == tab
        n = 540000 - 540000 % Cc
        assert describe(nat.hip_lib, n, 32, Cc, depth, 0) == (OK, f"k_noise_moments_u16<C={Cc},tab={tab},bits={depth}>")
        assert engine.noise_moments_kernel(n, 32, Cc, depth) == f"k_noise_moments_u16<C={Cc},tab={tab},bits={depth}>"
        for v in (LDS, GLOBAL, WINDOW):
            applies = v in variants(depth, Cc)
            for name, lib in _libs():
                rc, text = describe(lib, n, 32, Cc, depth, v)
                assert rc == (OK if applies else EUNSUP), (name, Cc, depth, v)
                assert text == ("" if not applies else f"k_noise_moments_u16<C={Cc},tab={TAB[v]},bits={depth}>" if name == "device" else
                                f"host_noise_moments<dn=u16,C={Cc},bits={depth}>"), (name, Cc, depth, v)
    for name, lib in _libs():
        buf = C.create_string_buffer(64)
        assert lib.hm_noise_moments_update_u16_describe(12, 2, 3, 12, 0, None, 0) == EINVAL, name
        assert lib.hm_noise_moments_update_u16_describe(12, 2, 3, 12, 0, buf, 0) == EINVAL, name
        assert describe(lib, 12, 2, 3, 8, 0) == (EINVAL, "") and describe(lib, 12, 2, 3, 12, 4) == (EINVAL, ""), name
        assert describe(lib, 12, 2, 5, 12, 0) == (EUNSUP, "") and describe(lib, 11, 2, 3, 12, 0) == (ESHAPE, ""), name
        assert describe(lib, 12, 0, 3, 12, 0) == (OK, "") and describe(lib, 0, 2, 3, 12, 0) == (OK, ""), name
    with pytest.raises(NotImplementedError):
        engine.noise_moments_kernel(12, 2, 3, 12, LDS)
    with nat.host_mode():
        assert engine.noise_moments_kernel(12, 2, 3, 12) == "host_noise_moments<dn=u16,C=3,bits=12>"


# ------------------------------------------------------------------------------------------------ 5: the Python surface
def check_python(dev):
    depth, shape = 12, (9, 11, 3)
    rng = np.random.default_rng(5)
    base = rng.integers(100, 3900, shape)
    a = [np.clip(base + rng.integers(-9, 10, shape), 0, 4095).astype(np.uint16) for _ in range(40)]
    b = [rng.integers(0, 4096, shape).astype(np.uint16) for _ in range(5)]
    # lists, callables, several videos, tensors; 45 frames in launches of 32 + 13 and of 7
    mom, mean = vp.compute_noise_moments([a, lambda: iter(b)], device=dev, bit_depth=depth)
    want_mean = vp.welford_algorithm([a, b], None, False, device=dev, bit_depth=depth)["mean"]
    assert mean.dtype == np.uint16 and np.array_equal(mean, want_mean)
    want = add_at_moments(a + b, mean, depth)
    assert mom.dtype == np.int64 and mom.shape == (4096, 3, 3) and np.array_equal(mom, want)
    mom7, _ = vp.compute_noise_moments(lambda: iter(a + b), device=dev, bit_depth=depth, frames_per_launch=7)
    assert np.array_equal(mom7, want)
    tm, tmean = vp.compute_noise_moments(iter([T(f, dev) for f in a + b]), mean_frame=T(mean, dev), device=dev, bit_depth=depth, as_numpy=False)
    assert isinstance(tm, torch.Tensor) and tm.device.type == torch.device(dev).type and tmean.dtype == torch.uint16     # one-shot is fine with a mean
    assert np.array_equal(tm.cpu().numpy(), want)
    gray, gmean = vp.compute_noise_moments([f[..., 0] for f in a], mean_frame=mean[..., 0], device=dev, bit_depth=depth)     # (H, W) frames
    assert gray.shape == (4096, 1, 3) and gmean.shape == (9, 11, 1)
    assert np.array_equal(gray, add_at_moments([f[..., :1] for f in a], mean[..., :1], depth))
    # what is refused
    with pytest.raises(ValueError, match="twice"):
        vp.compute_noise_moments(iter(a), device=dev, bit_depth=depth)
    with pytest.raises(ValueError, match="twice"):
        vp.compute_noise_moments([a, iter(b)], device=dev, bit_depth=depth)
    for bad in (None, 8, 17, 12.0, True):
        with pytest.raises(ValueError, match="bit_depth"):
            vp.compute_noise_moments(a, mean_frame=mean, device=dev, bit_depth=bad)
        with pytest.raises(ValueError, match="bit_depth"):
            vp.noise_moments_to_STD_data(mom, bad, device=dev)
    with pytest.raises(ValueError, match="bit_depth"):
        vp.compute_noise_moments([f.astype(np.uint8) for f in a[:3]], mean_frame=mean, device=dev, bit_depth=depth)      # uint8 frames with a depth
    with pytest.raises(ValueError, match="bit_depth"):
        vp.compute_noise_moments([f.astype(np.uint8) for f in a[:3]], device=dev, bit_depth=depth)
    with pytest.raises(ValueError, match="bit_depth"):
        vp.compute_noise_moments(a, mean_frame=mean.astype(np.uint8), device=dev, bit_depth=depth)                       # a uint8 mean frame
    with pytest.raises(ValueError, match="shape"):
        vp.compute_noise_moments(a, mean_frame=mean[:, :5], device=dev, bit_depth=depth)
    with pytest.raises(ValueError, match="4096"):
        vp.noise_moments_to_STD_data(mom[:256], depth, device=dev)
    with pytest.raises(TypeError):
        vp.noise_moments_to_STD_data(mom.astype(np.float64), depth, device=dev)
    with pytest.raises((TypeError, ValueError)):
        vp.compute_noise_profiles([a[:3]], device=dev)                                                                   # the profiles stay 8-bit
    # the engine's functions: nothing is changed by a refused call
    e = eng(dev)
    state, fd, md = T(np.zeros((4096, 3, 3), np.int64), dev), [T(f, dev) for f in a[:3]], T(mean, dev)
    with pytest.raises(ValueError):
        e.noise_moments_update(fd, md, state, depth, variant=4)
    with pytest.raises(NotImplementedError):
        e.noise_moments_update(fd, md, state, depth, variant=LDS)                                                        # 12 bits, C = 3: no fit
    with pytest.raises(ValueError, match="bit_depth"):
        e.noise_moments_update(fd, md, state, 8)
    with pytest.raises(ValueError, match="bit_depth"):
        e.noise_moments_update([f.to(torch.uint8) for f in fd], md, state, depth)
    with pytest.raises(ValueError, match="bit_depth"):
        e.noise_moments_update(fd, md.to(torch.uint8), state, depth)
    with pytest.raises(ValueError):
        e.noise_moments_update(fd, md, state, 11)                                                                        # 2048 rows wanted
    with pytest.raises(ValueError):
        e.noise_moments_update(fd[:2] + [fd[2][:, :5]], md, state, depth)
    with pytest.raises(TypeError):
        e.noise_moments_update(fd, md, state.to(torch.int32), depth)
    with pytest.raises(ValueError):
        e.noise_moments_std(state, 11)
    assert not state.cpu().numpy().any()
    e.noise_moments_update(fd, md, state, depth, variant=None)
    assert np.array_equal(state.cpu().numpy(), add_at_moments(a[:3], mean, depth))


def test_python_surface():
    check_python("cpu")
