"""The per-level noise moments of uint16 frames and the STD table from them on the MI355X (k_noise_moments_u16, k_noise_moments_std): the
checks of tests/test_noise_moments_host.py with device tensors. The device moments are compared with the HOST build's, integer for integer,
in every placement that exists for a case; the table with the exact oracle of that file, to its derived bound of 8 * 2^-53."""
import ctypes as C

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine
from camera_linearity_amd import video_processing as vp
import test_noise_moments_host as nm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host_moments(frames, mean, depth):
    """the host build's moments of (unmasked) frames: the reference of the device kernels"""
    mom = torch.zeros((2 ** depth, mean.shape[-1], 3), dtype=torch.int64)
    nm.eng("cpu").noise_moments_update([torch.from_numpy(np.ascontiguousarray(f)) for f in frames], torch.from_numpy(np.ascontiguousarray(mean)), mom, depth)
    return mom.numpy()


@pytest.mark.parametrize("depth", nm.DEPTHS)
@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
def test_moments_match_the_host_build(Cc, depth):
    """shape (37, 41, C): 1517 C elements, no multiple of 8 for odd C, the channel phase differs per unit; LDS at 9 and 11 bits with C = 3
    and at 12 bits with C = 1, no LDS at 12 bits with C = 3 and at 16 bits, as the fit rule has it; global atomics and the window everywhere"""
    assert nm.variants(9, 3) == [0, 1, 2, 3] and nm.variants(11, 3) == [0, 1, 2, 3] and nm.variants(12, 1) == [0, 1, 2, 3]
    assert nm.variants(12, 3) == [0, 2, 3] and nm.variants(16, 1) == [0, 2, 3]
    nm.check_moments(DEV, (37, 41), Cc, depth, host_moments)


# (shape, depth, frames): 70 000 elements - nine workgroups of the LDS form, 35 of the global form; 4 320 000 elements = 540 000 units, more
# than one pass of the LDS form's grid (256 workgroups of 1024 lanes) and of the global form's (2048 workgroups of 256)
LARGE = [((100, 175, 4), 10, 32), ((1200, 1200, 3), 11, 2)]


@pytest.mark.parametrize("shape,depth,N", LARGE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_several_workgroups_and_the_grid_stride_loop(shape, depth, N):
    n = 2 ** depth
    rng = np.random.default_rng(shape[0] + depth)
    base = rng.integers(0, n, shape)
    frames = np.clip(base + np.around(rng.standard_normal((N,) + shape) * 6), 0, n - 1).astype(np.uint16)
    mean = base.astype(np.uint16)
    want = host_moments(list(frames), mean, depth)
    assert want[:, :, 0].sum() == N * mean.size
    assert nm.variants(depth, shape[2]) == [0, nm.LDS, nm.GLOBAL, nm.WINDOW]
    fd, md = [nm.T(f, DEV) for f in frames], nm.T(mean, DEV)
    for v in (0, nm.LDS, nm.GLOBAL, nm.WINDOW):
        assert np.array_equal(nm.run_update(DEV, fd, md, depth, v).cpu().numpy(), want), v
    const = nm.T(np.full_like(mean, 77), DEV)                               # every lane on the same C levels
    want_const = host_moments(list(frames), np.full_like(mean, 77), depth)
    for v in (nm.LDS, nm.GLOBAL, nm.WINDOW):
        assert np.array_equal(nm.run_update(DEV, fd, const, depth, v).cpu().numpy(), want_const), v


def test_forced_lds_one_bit_above_the_fit_rule_is_refused_at_the_call():
    """HM_EUNSUPPORTED from the entry point itself, on device pointers, and nothing is launched: the state keeps its content"""
    for Cc, depth in ((1, 13), (2, 12), (3, 12), (4, 11)):
        assert nm.fits_lds(depth - 1, Cc) and not nm.fits_lds(depth, Cc)
        shape = (5, 8, Cc)
        frame = torch.full(shape, 3, dtype=torch.int16, device=DEV).view(torch.uint16)
        mom = torch.full((2 ** depth, Cc, 3), 5, dtype=torch.int64, device=DEV)
        ptrs = (C.c_void_p * 1)(frame.data_ptr())
        stream = torch.cuda.current_stream(DEV).cuda_stream
        calls = nat.hip_lib.calls["hm_noise_moments_update_u16"]
        assert nat.hip_lib.hm_noise_moments_update_u16(ptrs, 1, frame.data_ptr(), frame.numel(), Cc, depth, mom.data_ptr(), nm.LDS,
                                                       stream) == nat.HM_EUNSUPPORTED
        assert nat.hip_lib.calls["hm_noise_moments_update_u16"] == calls + 1
        with pytest.raises(NotImplementedError):
            engine.noise_moments_update([frame], frame, mom, depth, variant=nm.LDS)
        torch.cuda.synchronize()
        assert bool((mom == 5).all())
        engine.noise_moments_update([frame], frame, mom, depth, variant=nm.GLOBAL)                          # the other placement serves it
        torch.cuda.synchronize()
        assert mom[3, :, 0].tolist() == [5 + 40] * Cc


def test_describe_names_the_placement_the_fit_rule_predicts():
    for Cc in (1, 2, 3, 4):
        for depth in range(9, 17):
            tab = "lds" if nm.fits_lds(depth, Cc) else "window"
            assert engine.noise_moments_kernel(1517 * Cc, 32, Cc, depth) == f"k_noise_moments_u16<C={Cc},tab={tab},bits={depth}>"


@pytest.mark.parametrize("depth,Cc", [(9, 1), (12, 3), (16, 3), (16, 4)])
def test_table_against_exact_oracle(depth, Cc):
    nm.check_table(DEV, depth, Cc)


def test_golden_profiles_and_std(golden):
    nm.check_golden(DEV, golden("noise"))


def test_python_surface():
    nm.check_python(DEV)


def test_end_to_end_12_bits():
    """40 noisy uint16 frames -> moments -> table -> std frames by linearize -> the fused uint16 merge: finite, and equal to the merge fed
    with table[DN] gathered in NumPy"""
    depth, n, shape = 12, 4096, (48, 64, 3)
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    scene = (200 + 3500 * (xx / shape[1]) * (0.6 + 0.4 * yy / shape[0]))[:, :, None] * np.array([1.0, 0.8, 0.6])
    video = [np.clip(np.around(scene + rng.standard_normal(shape) * (2 + np.sqrt(scene) / 4)), 0, n - 1).astype(np.uint16) for _ in range(40)]
    mom, mean = vp.compute_noise_moments(video, bit_depth=depth)
    mom_h, mean_h = vp.compute_noise_moments(video, device="cpu", bit_depth=depth)
    assert np.array_equal(mean, mean_h) and np.array_equal(mom, mom_h)
    assert mom[:, :, 0].sum() == 40 * mean.size
    table = vp.noise_moments_to_STD_data(mom, depth)
    assert table.shape == (n, 3) and np.isfinite(table).sum() == np.count_nonzero(mom[:, :, 0])
    # three exposures of the scene; every DN a level of the video's mean frame, so every std is a populated row of the table
    exposures = [1.0, 2.0, 4.0]
    frames = [np.ascontiguousarray(np.roll(mean, k, axis=1)) for k in range(3)]
    icrf = np.repeat((np.arange(n) / (n - 1))[:, None] ** 1.2, 3, axis=1)
    diff = np.gradient(icrf, axis=0) * (n - 1)
    fd = [nm.T(f, DEV) for f in frames]
    stds = [engine.linearize(f, None, table, bit_depth=depth)[0] for f in fd]
    gathered = [table[f.astype(np.int64), np.arange(3)] for f in frames]
    for s, g in zip(stds, gathered):
        assert np.isfinite(g).all() and np.array_equal(s.cpu().numpy(), g)
    out = engine.merge(fd, exposures, icrf, diff, stds, bit_depth=depth)
    ref = engine.merge(fd, exposures, icrf, diff, [nm.T(g, DEV) for g in gathered], bit_depth=depth)
    torch.cuda.synchronize()
    for key in ("val", "std"):
        got = out[key].cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got, ref[key].cpu().numpy()), key


def test_update_is_capturable_and_adds_twice_on_two_replays():
    depth, shape = 11, (64, 96, 3)
    rng = np.random.default_rng(4)
    base = rng.integers(0, 2 ** depth, shape)
    mean = nm.T(base.astype(np.uint16), DEV)
    frames = [nm.T(np.clip(base + rng.integers(-3, 4, shape), 0, 2 ** depth - 1).astype(np.uint16), DEV) for _ in range(20)]
    for v in (nm.LDS, nm.GLOBAL, nm.WINDOW):
        once = nm.run_update(DEV, frames, mean, depth, v)                   # warm-up outside the capture
        state = torch.zeros_like(once)
        s = torch.cuda.Stream(DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            engine.noise_moments_update(frames, mean, state, depth, v)
        torch.cuda.current_stream(DEV).wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            engine.noise_moments_update(frames, mean, state, depth, v)
        state.zero_()
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(state, 2 * once), v
