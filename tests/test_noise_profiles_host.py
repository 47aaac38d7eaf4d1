"""Noise profiles and the per-DN STD table on the HOST build (libhdrmerge_host.so, device="cpu"): against the reference's own
output (tests/golden/noise.npz, make_golden_noise.py) and an np.bincount restatement of the histogram. No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from camera_linearity_amd import _native as nat
from camera_linearity_amd import video_processing as vp


def bincount_profiles(frames, mean):
    """profiles[m, f, c] = #(mean == m, frame == f, channel c) over all frames: np.add.at of :104 as one bincount."""
    mean = mean.reshape(-1, mean.shape[-1]) if mean.ndim == 3 else mean.reshape(-1, 1)
    Cc = mean.shape[1]
    out = np.zeros((256, 256, Cc), dtype=np.int64)
    for f in frames:
        f = f.reshape(-1, Cc)
        for c in range(Cc):
            out[:, :, c] += np.bincount(mean[:, c].astype(np.int64) * 256 + f[:, c], minlength=65536).reshape(256, 256)
    return out


def assert_std_equal(a, b):
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    np.testing.assert_allclose(a[ok], b[ok], rtol=1e-13, atol=0)


def test_host_profiles_match_reference(golden):
    z = golden("noise")
    prof, mean = vp.compute_noise_profiles([list(z["clip_a"]), list(z["clip_b"])], device="cpu")
    assert prof.dtype == np.int64 and prof.shape == (256, 256, 3)
    assert np.array_equal(mean, z["mean"])
    assert np.array_equal(prof, z["profiles"])


def test_host_std_table_matches_reference(golden):
    z = golden("noise")
    assert_std_equal(vp.noise_profiles_to_STD_data(z["profiles"], device="cpu"), z["std"])
    for c in range(3):
        assert_std_equal(vp._calculate_STD(z["profiles"][:, :, c], device="cpu"), z["std"][:, c])


def test_host_clean_edges_matches_reference(golden):
    z = golden("noise")
    p = z["profiles"].copy()
    assert vp.clean_data_edges(p, device="cpu") is p                  # in place, returned
    assert np.array_equal(p, z["cleaned"])
    for a_in, a_out in zip(z["extra_in"], z["extra_out"]):
        a = a_in.copy()
        vp.clean_data_edges(a, device="cpu")
        assert np.array_equal(a, a_out)


@pytest.mark.parametrize("C,fpl", [(1, 1), (3, 7), (4, 32), (3, 32)])
def test_host_profiles_match_bincount(C, fpl):
    rng = np.random.default_rng(100 + C * 10 + fpl)
    h, w = 19, 23
    base = rng.integers(0, 256, (h, w, C))
    a = [np.clip(base + rng.integers(-5, 6, (h, w, C)), 0, 255).astype(np.uint8) for _ in range(11)]
    b = [rng.integers(0, 256, (h, w, C), dtype=np.uint8) for _ in range(6)]
    frames = a + b
    prof, mean = vp.compute_noise_profiles([a, lambda: iter(b)], device="cpu", frames_per_launch=fpl)
    ref_mean = vp.welford_algorithm([a, b], device="cpu")["mean"]
    assert np.array_equal(mean, ref_mean)
    assert np.array_equal(prof, bincount_profiles(frames, mean))
    assert all(prof[..., c].sum() == len(frames) * h * w for c in range(C))


def test_host_callable_source_and_given_mean():
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (9, 13), dtype=np.uint8) for _ in range(5)]
    mean = rng.integers(0, 256, (9, 13), dtype=np.uint8)
    prof, m = vp.compute_noise_profiles(lambda: iter(frames), device="cpu")
    assert prof.shape == (256, 256, 1) and m.shape == (9, 13, 1)
    assert np.array_equal(prof, bincount_profiles(frames, m[..., 0]))
    prof2, m2 = vp.compute_noise_profiles(iter(frames), mean_frame=mean, device="cpu")    # one-shot is fine with mean_frame
    assert np.array_equal(m2[..., 0], mean)
    assert np.array_equal(prof2, bincount_profiles(frames, mean))


def test_one_shot_iterator_without_mean_raises():
    frames = (np.zeros((4, 4, 3), np.uint8) for _ in range(3))
    with pytest.raises(ValueError, match="twice"):
        vp.compute_noise_profiles(frames, device="cpu")
    with pytest.raises(ValueError, match="twice"):
        vp.compute_noise_profiles([[np.zeros((4, 4, 3), np.uint8)], iter([np.zeros((4, 4, 3), np.uint8)])], device="cpu")


def test_api_argument_errors():
    with pytest.raises(ValueError):
        vp.noise_profiles_to_STD_data(np.zeros((255, 256, 3), np.int64), device="cpu")
    with pytest.raises(TypeError):
        vp.clean_data_edges(np.zeros((256, 256), np.float64), device="cpu")
    with pytest.raises(ValueError):
        vp._calculate_STD(np.zeros((256, 256, 2), np.int64), device="cpu")
    with pytest.raises(ValueError):
        vp.compute_noise_profiles([np.zeros((4, 4, 3), np.uint8)], mean_frame=np.zeros((4, 5, 3), np.uint8), device="cpu")


def test_entry_point_validation_host():
    """hm_noise_profile_*: null pointers and n_frames > HM_MAX_FRAMES -> HM_EINVAL, C > 4 -> HM_EUNSUPPORTED, n % C -> HM_ESHAPE."""
    h = nat.host_lib()
    fr = np.zeros(12, np.uint8)
    prof = np.zeros((256, 256, 4), np.int64)
    ptrs = (C.c_void_p * 33)(*([fr.ctypes.data] * 33))
    upd = lambda p, n, m, ne, c, out: h.hm_noise_profile_update(p, n, m, ne, c, out, None, 0, None)   # noqa: E731
    assert upd(ptrs, 33, fr.ctypes.data, 12, 3, prof.ctypes.data) == nat.HM_EINVAL
    assert upd(None, 1, fr.ctypes.data, 12, 3, prof.ctypes.data) == nat.HM_EINVAL
    assert upd(ptrs, 1, None, 12, 3, prof.ctypes.data) == nat.HM_EINVAL
    assert upd(ptrs, 1, fr.ctypes.data, 12, 3, None) == nat.HM_EINVAL
    assert upd((C.c_void_p * 1)(None), 1, fr.ctypes.data, 12, 3, prof.ctypes.data) == nat.HM_EINVAL
    assert upd(ptrs, 1, fr.ctypes.data, 12, 5, prof.ctypes.data) == nat.HM_EUNSUPPORTED
    assert upd(ptrs, 1, fr.ctypes.data, 12, 0, prof.ctypes.data) == nat.HM_EINVAL
    assert upd(ptrs, 1, fr.ctypes.data, 10, 3, prof.ctypes.data) == nat.HM_ESHAPE
    assert not prof.any()
    edges = np.linspace(0, 1, 256)
    out = np.zeros(256 * 4)
    assert h.hm_noise_profile_std(None, 3, edges.ctypes.data, out.ctypes.data, None) == nat.HM_EINVAL
    assert h.hm_noise_profile_std(prof.ctypes.data, 3, None, out.ctypes.data, None) == nat.HM_EINVAL
    assert h.hm_noise_profile_std(prof.ctypes.data, 3, edges.ctypes.data, None, None) == nat.HM_EINVAL
    assert h.hm_noise_profile_std(prof.ctypes.data, 5, edges.ctypes.data, out.ctypes.data, None) == nat.HM_EUNSUPPORTED
    assert h.hm_noise_profile_clean_edges(None, 3, None) == nat.HM_EINVAL
    assert h.hm_noise_profile_clean_edges(prof.ctypes.data, 5, None) == nat.HM_EUNSUPPORTED
    assert h.hm_noise_profile_algorithmic_bytes(32, 1920 * 1080 * 3, 3) == 1920 * 1080 * 3 * 33 + 2 * 65536 * 3 * 8


def test_device_entry_point_validation_without_a_device():
    """The device build validates before any HIP call: these return without touching a GPU."""
    lib = nat.hip_lib
    fr = (C.c_void_p * 33)(*([16] * 33))
    assert lib.hm_noise_profile_update(fr, 33, 16, 12, 3, 16, None, 0, None) == nat.HM_EINVAL
    assert lib.hm_noise_profile_update(None, 1, 16, 12, 3, 16, None, 0, None) == nat.HM_EINVAL
    assert lib.hm_noise_profile_update(fr, 1, None, 12, 3, 16, None, 0, None) == nat.HM_EINVAL
    assert lib.hm_noise_profile_update(fr, 1, 16, 12, 3, None, None, 0, None) == nat.HM_EINVAL
    assert lib.hm_noise_profile_update(fr, 1, 16, 12, 5, 16, None, 0, None) == nat.HM_EUNSUPPORTED
    assert lib.hm_noise_profile_update(fr, 1, 16, 10, 3, 16, None, 0, None) == nat.HM_ESHAPE
    assert lib.hm_noise_profile_std(None, 3, 16, 16, None) == nat.HM_EINVAL
    assert lib.hm_noise_profile_std(16, 5, 16, 16, None) == nat.HM_EUNSUPPORTED
    assert lib.hm_noise_profile_clean_edges(None, 3, None) == nat.HM_EINVAL
    assert lib.hm_noise_profile_clean_edges(16, 5, None) == nat.HM_EUNSUPPORTED
    assert lib.hm_noise_profile_workspace_bytes(1920 * 1080 * 3, 3) == 0
