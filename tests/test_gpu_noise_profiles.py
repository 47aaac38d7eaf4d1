"""Noise profiles and the per-DN STD table on the MI355X (hm_noise.hip): exact against the reference's own output
(tests/golden/noise.npz), against an np.bincount restatement of the histogram, and against the host build."""
import ctypes as C

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import video_processing as vp
from camera_linearity_amd.image_set import ImageSet

from test_noise_profiles_host import assert_std_equal, bincount_profiles

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def test_device_profiles_match_reference(golden):
    z = golden("noise")
    prof, mean = vp.compute_noise_profiles([list(z["clip_a"]), list(z["clip_b"])])
    assert np.array_equal(mean, z["mean"])
    assert np.array_equal(prof, z["profiles"])
    assert_std_equal(vp.noise_profiles_to_STD_data(prof), z["std"])
    p = z["profiles"].copy()
    assert vp.clean_data_edges(p) is p
    assert np.array_equal(p, z["cleaned"])
    for a_in, a_out in zip(z["extra_in"], z["extra_out"]):
        a = torch.as_tensor(a_in, device=DEV)
        assert vp.clean_data_edges(a) is a
        assert np.array_equal(a.cpu().numpy(), a_out)


def test_device_1080p_sigma2_70_frames():
    """1920 x 1080 x 3, sigma 2 DN, 70 frames = launches of 32 + 32 + 6."""
    g = torch.Generator(device=DEV).manual_seed(5)
    h, w = 1080, 1920
    yy = torch.linspace(0, 1, h, device=DEV)[:, None, None]
    xx = torch.linspace(0, 1, w, device=DEV)[None, :, None]
    scene = 255 * (0.5 * yy + 0.5 * xx) * torch.tensor([0.6, 0.8, 1.1], device=DEV)
    frames = [torch.clamp(torch.round(scene + 2 * torch.randn((h, w, 3), device=DEV, generator=g)), 0, 255).to(torch.uint8)
              for _ in range(70)]
    prof, mean = vp.compute_noise_profiles(frames, as_numpy=False)
    assert prof.device == DEV and mean.dtype == torch.uint8
    host = [f.cpu().numpy() for f in frames]
    ref_mean = vp.welford_algorithm(frames)["mean"]
    assert np.array_equal(mean.cpu().numpy(), ref_mean)
    assert np.array_equal(prof.cpu().numpy(), bincount_profiles(host, ref_mean))


@pytest.mark.parametrize("shape", [(257, 131, 1), (33, 47, 4), (31, 29, 2)])
def test_device_odd_geometry(shape):
    rng = np.random.default_rng(sum(shape))
    base = rng.integers(0, 256, shape)
    frames = [np.clip(base + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8) for _ in range(37)]
    prof, mean = vp.compute_noise_profiles(frames)
    assert np.array_equal(prof, bincount_profiles(frames, mean))


def test_device_out_of_band_uniform_random():
    rng = np.random.default_rng(9)
    mean = rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(40)]
    prof, m = vp.compute_noise_profiles(frames, mean_frame=mean)
    assert np.array_equal(m, mean)
    assert np.array_equal(prof, bincount_profiles(frames, mean))


def test_device_constant_frame():
    n, h, w = 64, 512, 384
    frame = torch.full((h, w, 3), 77, dtype=torch.uint8, device=DEV)
    prof, mean = vp.compute_noise_profiles([frame] * n)
    assert (mean == 77).all()
    expect = np.zeros((256, 256, 3), np.int64)
    expect[77, 77, :] = n * h * w
    assert np.array_equal(prof, expect)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_native_unaligned_pointers_and_ragged_length(offset):
    """Frame and mean pointers offset by 1-3 bytes, n_elems not a multiple of 16 (the byte-load path and the ragged tail)."""
    rng = np.random.default_rng(offset)
    Cc, n = 3, 3 * 4099
    mean = rng.integers(0, 256, n, dtype=np.uint8)
    frames = [np.clip(mean.astype(int) + rng.integers(-30, 31, n), 0, 255).astype(np.uint8) for _ in range(9)]
    buf_m = torch.zeros(n + 16, dtype=torch.uint8, device=DEV)
    buf_m[offset:offset + n] = torch.as_tensor(mean, device=DEV)
    bufs = []
    for k, f in enumerate(frames):
        b = torch.zeros(n + 16, dtype=torch.uint8, device=DEV)
        o = (offset + k) % 4
        b[o:o + n] = torch.as_tensor(f, device=DEV)
        bufs.append((b, o))
    prof = torch.zeros((256, 256, Cc), dtype=torch.int64, device=DEV)
    ptrs = (C.c_void_p * len(bufs))(*[b.data_ptr() + o for b, o in bufs])
    stream = torch.cuda.current_stream(DEV).cuda_stream
    nat.check(nat.hip_lib.hm_noise_profile_update(ptrs, len(bufs), buf_m.data_ptr() + offset, n, Cc, prof.data_ptr(), None, 0, stream))
    torch.cuda.synchronize()
    assert np.array_equal(prof.cpu().numpy(), bincount_profiles(frames, mean.reshape(1, -1, Cc)))


def test_updates_accumulate_and_graph_replay():
    from camera_linearity_amd import engine
    rng = np.random.default_rng(4)
    mean = torch.as_tensor(rng.integers(0, 256, (64, 96, 3), dtype=np.uint8), device=DEV)
    fa = [torch.as_tensor(np.clip(mean.cpu().numpy() + rng.integers(-3, 4, (64, 96, 3)), 0, 255).astype(np.uint8), device=DEV)
          for _ in range(20)]
    fb = [torch.as_tensor(rng.integers(0, 256, (64, 96, 3), dtype=np.uint8), device=DEV) for _ in range(13)]
    pa = torch.zeros((256, 256, 3), dtype=torch.int64, device=DEV)
    pb = torch.zeros_like(pa)
    both = torch.zeros_like(pa)
    engine.noise_profile_update(fa, mean, pa)
    engine.noise_profile_update(fb, mean, pb)
    engine.noise_profile_update(fa, mean, both)
    engine.noise_profile_update(fb, mean, both)
    assert torch.equal(both, pa + pb)

    g_prof = torch.zeros_like(pa)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        engine.noise_profile_update(fa, mean, g_prof)          # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(s)
    g_prof.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        engine.noise_profile_update(fa, mean, g_prof)
    g_prof.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_prof, 2 * pa)


def test_device_matches_host_build():
    rng = np.random.default_rng(12)
    base = rng.integers(0, 256, (50, 70, 3))
    frames = [np.clip(base + np.around(rng.standard_normal(base.shape) * 4), 0, 255).astype(np.uint8) for _ in range(45)]
    pd, md = vp.compute_noise_profiles(frames)
    ph, mh = vp.compute_noise_profiles(frames, device="cpu")
    assert np.array_equal(md, mh) and np.array_equal(pd, ph)
    assert_std_equal(vp.noise_profiles_to_STD_data(pd), vp.noise_profiles_to_STD_data(ph, device="cpu"))
    cd, ch = vp.clean_data_edges(pd.copy()), vp.clean_data_edges(ph.copy(), device="cpu")
    assert np.array_equal(cd, ch)


def test_end_to_end_std_table_through_image_set():
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (40, 60, 3))
    frames = [np.clip(base + np.around(rng.standard_normal(base.shape) * 3), 0, 255).astype(np.uint8) for _ in range(30)]
    prof, _ = vp.compute_noise_profiles(frames)
    table = vp.noise_profiles_to_STD_data(prof)
    assert table.shape == (256, 3) and table.dtype == np.float64
    u8 = rng.integers(0, 256, (40, 60, 3), dtype=np.uint8)
    expect = table[u8, np.arange(3)]
    for use_cupy in (True, False):                      # the device backend, then the host backend
        got = ImageSet(value=u8, use_cupy=use_cupy).calculate_numerical_STD(table)
        got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
        assert np.array_equal(got, expect, equal_nan=True)
