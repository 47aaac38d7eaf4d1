"""TIFF strips encoded on the MI355X (hm_tiff_encode.hip through the raw C ABI, tiff_io.imwrite_device and ImageSet.save_*), against
the host build's hm_tiff_encode_strips - which tests/test_tiff_encode_host.py pins against lzw_encode byte for byte on a box without a
GPU - and against tiff_io.imwrite's files. All inputs are valid."""
import itertools

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import tiff_io as T
from camera_linearity_amd.image_set import ImageSet

from test_tiff_device_host import bgr, family_image
from test_tiff_encode_host import abi_encode, data_kinds, pillow_array, quantise_image, strip_cases

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def assert_device_equals_host(name, img, kind, divisor, rps, compression, predictor):
    want = abi_encode(nat.host_lib(), img, kind, divisor, rps, compression, predictor)
    got = abi_encode(nat.hip_lib, img, kind, divisor, rps, compression, predictor, on_device=True)
    assert want[3] == 0 and got[3] == 0, name
    assert np.array_equal(got[1], want[1]), f"{name}: offsets"
    assert np.array_equal(got[2], want[2]), f"{name}: counts"
    assert got[0].tobytes() == want[0].tobytes(), f"{name}: payload"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the C ABI against the host build
# ---------------------------------------------------------------------------------------------------------------------
def test_strip_family_is_byte_equal_to_the_host_build():
    """The cases of the host test: strip sizes 1 .. 98 304 of the four data kinds, around the first Clear, 1 / 3 / 4 samples, both
    predictors, short last strips, 1 x 1, float64, quantised."""
    n = 0
    for name, img, kind, rps, predictor in strip_cases():
        assert_device_equals_host(name, img, kind, 3.0 if kind == 2 else 1.0, rps, 5, predictor)
        n += 1
    assert n > 80


def test_strips_around_the_fetch_and_flush_sizes():
    """The kernel stages no strip in LDS; what it does in blocks is the input fetch (256 bytes, the next 256 in flight) and the output
    flush (64 words = 256 bytes). Strips one byte below, at and above 256, 512 and 768 bytes, of noise (output longer than input: the
    flush boundary is crossed early) and of zeros (a handful of output words: only the final partial flush runs)."""
    for n in (255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025):
        for name in ("noise", "zeros", "ramp"):
            assert_device_equals_host(f"{name}{n}", data_kinds(n)[name].reshape(1, n), 0, 1.0, 1, 5, 1)
    noise = data_kinds(170 * 3)["noise"]                              # 170 bytes of noise give about 256 bytes of stream: one full flush
    for n in range(165, 175):
        assert_device_equals_host(f"flush{n}", noise[:n].reshape(1, n), 0, 1.0, 1, 5, 1)


@pytest.mark.parametrize("compression", [1, 5])
def test_pack_widths_kinds_and_predictors(compression):
    """Widths around the pack kernel's 64-pixel step, every source kind, samples and predictor, several rows per strip."""
    rng = np.random.default_rng(12)
    for W, samples in itertools.product((1, 63, 64, 65, 129), (1, 3, 4)):
        u = family_image((9, W), samples, seed=W)
        for predictor in (1, 2):
            assert_device_equals_host(f"u8 w{W} s{samples} p{predictor}", u, 0, 1.0, 4, compression, predictor)
        f = rng.random((9, W, samples)) * 2.5
        f = f[:, :, 0] if samples == 1 else f
        assert_device_equals_host(f"f64 w{W} s{samples}", f, 1, 1.0, 4, compression, 1)
        for predictor in (1, 2):
            assert_device_equals_host(f"q w{W} s{samples} p{predictor}", f, 2, 2.5, 4, compression, predictor)


def test_more_strips_than_the_per_strip_kernels_have_workgroups():
    """2^16 + 3 one-row strips: the LZW and the compaction kernel launch at most 2^16 workgroups and loop over the rest."""
    H = (1 << 16) + 3
    img = (np.arange(H * 5, dtype=np.int64) * 7 % 251).astype(np.uint8).reshape(H, 5)
    assert_device_equals_host("65539 strips", img, 0, 1.0, 1, 5, 1)
    got = abi_encode(nat.hip_lib, img, 0, 1.0, 1, 5, 2, on_device=True)
    assert got[3] == 0 and (got[2] > 0).all() and (np.diff(got[1]) == 16).all()


@pytest.mark.parametrize("d", [1.0, 2.0, 3.7, 255.0])
def test_quantisation_on_the_device_with_ties(d):
    img, n_ties = quantise_image(d)
    assert n_ties >= 200
    payload, _, _, rc = abi_encode(nat.hip_lib, img, 2, d, 4, 1, 1, on_device=True)
    assert rc == 0
    want = np.around((img / d) * 255.0).astype(np.uint8)
    assert np.array_equal(payload.reshape(img.shape), bgr(want))
    odd = np.array([[np.nan, np.inf, -np.inf, -1.0 / 255.0, 0.0, 1.0, 256.0 / 255.0, 1e300]], dtype=np.float64)
    payload, _, _, rc = abi_encode(nat.hip_lib, odd, 2, 1.0, 1, 1, 1, on_device=True)
    assert rc == 0 and list(payload) == [0, 0, 0, 255, 0, 255, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# 2. files
# ---------------------------------------------------------------------------------------------------------------------
def file_tensors():
    rng = np.random.default_rng(21)
    for W in (1, 65, 129):
        for samples in (1, 3, 4):
            yield f"u8s{samples}w{W}", family_image((70, W), samples, seed=W + samples)
        for samples in (1, 3):
            f = rng.random((70, W, samples)) * 4.0
            yield f"f8s{samples}w{W}", f[:, :, 0] if samples == 1 else f


def test_uncompressed_device_files_are_byte_identical_to_imwrite(tmp_path):
    calls = nat.hip_lib.calls["hm_tiff_encode_strips"]
    n = 0
    for name, img in file_tensors():
        T.imwrite(tmp_path / "host.tif", img)
        assert T.imwrite_device(tmp_path / "dev.tif", torch.from_numpy(img).to(DEV))
        assert (tmp_path / "dev.tif").read_bytes() == (tmp_path / "host.tif").read_bytes(), name
        n += 1
    assert nat.hip_lib.calls["hm_tiff_encode_strips"] == calls + n


@pytest.mark.parametrize("predictor", [1, 2])
def test_lzw_device_files_read_back_everywhere(tmp_path, predictor):
    pytest.importorskip("PIL.Image")
    for name, img in file_tensors():
        if img.dtype != np.uint8 and predictor == 2:
            continue
        p = tmp_path / f"{name}.tif"
        T.imwrite_device(p, torch.from_numpy(img).to(DEV), compression=5, predictor=predictor)
        T.imwrite(tmp_path / "host.tif", img, compression=5, predictor=predictor)
        assert p.read_bytes() == (tmp_path / "host.tif").read_bytes(), name         # the same strips, so the same file
        assert np.array_equal(T.imread(p, T.IMREAD_UNCHANGED), img), name
        got = T.imread_device(p, T.IMREAD_UNCHANGED, device=DEV).cpu().numpy()
        assert got.dtype == img.dtype and np.array_equal(got, img), name
        assert np.array_equal(pillow_array(p), bgr(img)), name


@pytest.mark.parametrize("compression", [1, 5])
def test_quantised_device_files(tmp_path, compression):
    for d in (1.0, 3.7):
        img, n_ties = quantise_image(d)
        assert n_ties >= 200
        p = tmp_path / "q.tif"
        T.imwrite_device(p, torch.from_numpy(img).to(DEV), compression=compression, quantize_divisor=d)
        want = np.around((img / d) * 255.0).astype(np.uint8)
        got = T.imread(p, T.IMREAD_UNCHANGED)
        assert got.dtype == np.uint8 and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. ImageSet.save_64bit / save_8bit
# ---------------------------------------------------------------------------------------------------------------------
def merged_set(tmp_path, with_std=True):
    """A 64 x 48 x 3 'merged' image with values above 1 (so save_8bit scales) and a std image with values above 1 too."""
    rng = np.random.default_rng(33)
    val = rng.random((64, 48, 3)) * 5.0 + np.add.outer(np.arange(64), np.arange(48))[:, :, None] / 20.0
    std = rng.random((64, 48, 3)) * 1.5 if with_std else None
    return ImageSet(file_path=tmp_path / "10ms bf 5x merged.tif", value=val, std=std, use_cupy=True)


def decoded(folder):
    return {p.name: T.imread(p, T.IMREAD_UNCHANGED) for p in sorted(folder.glob("*.tif"))}


def assert_same_files(a, b):
    assert a.keys() == b.keys() and len(a) > 0
    for name in a:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape and np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("separate_channels", [False, True])
def test_save_64bit_device_encode(tmp_path, separate_channels):
    s = merged_set(tmp_path)
    (tmp_path / "h").mkdir()
    (tmp_path / "d").mkdir()
    s.save_64bit(tmp_path / "h" / "m.tif", is_HDR=True, separate_channels=separate_channels)
    calls = nat.hip_lib.calls["hm_tiff_encode_strips"]
    s.save_64bit(tmp_path / "d" / "m.tif", is_HDR=True, separate_channels=separate_channels, device_encode=True)
    n_files = 6 if separate_channels else 2
    assert nat.hip_lib.calls["hm_tiff_encode_strips"] == calls + n_files
    assert_same_files(decoded(tmp_path / "d"), decoded(tmp_path / "h"))
    for p in (tmp_path / "d").glob("*.tif"):
        assert p.read_bytes() == (tmp_path / "h" / p.name).read_bytes(), p.name


@pytest.mark.parametrize("force_8_bit,compression", [(False, 1), (False, 5), (True, 1), (True, 5)])
def test_save_8bit_device_encode(tmp_path, force_8_bit, compression):
    s = merged_set(tmp_path)
    (tmp_path / "h").mkdir()
    (tmp_path / "d").mkdir()
    s.save_8bit(tmp_path / "h" / "m.tif", force_8_bit=force_8_bit, compression=compression)
    calls = nat.hip_lib.calls["hm_tiff_encode_strips"]
    s.save_8bit(tmp_path / "d" / "m.tif", force_8_bit=force_8_bit, device_encode=True, compression=compression)
    assert nat.hip_lib.calls["hm_tiff_encode_strips"] == calls + 2
    got, want = decoded(tmp_path / "d"), decoded(tmp_path / "h")
    assert_same_files(got, want)
    assert got["m.tif"].dtype == np.uint8 and got["m.tif"].max() == 255
    assert got["m STD.tif"].dtype == (np.uint8 if force_8_bit else np.float64)


def test_save_8bit_of_a_frame_that_still_holds_its_dns(tmp_path):
    dn = family_image((64, 48), 3, seed=3)
    s = ImageSet(file_path=tmp_path / "10ms bf 5x frame.tif", value=dn, use_cupy=True)
    s.save_8bit(tmp_path / "h.tif")
    calls = nat.hip_lib.calls["hm_tiff_encode_strips"]
    s.save_8bit(tmp_path / "d.tif", device_encode=True)
    assert nat.hip_lib.calls["hm_tiff_encode_strips"] == calls + 1
    assert (tmp_path / "d.tif").read_bytes() == (tmp_path / "h.tif").read_bytes()
    assert np.array_equal(T.imread(tmp_path / "d.tif", T.IMREAD_UNCHANGED), dn)


@pytest.mark.parametrize("top", [199, 1])
def test_save_8bit_of_a_uint8_value_image_that_is_not_a_dn_frame(tmp_path, top):
    """A uint8 `val` that did not come through from_dn: its values ARE the DNs (`.val` is not DN / 255), so save_8bit scales them by
    their maximum like any other image - 199 becomes 255 - although `.dn` hands the tensor out. Only a from_dn frame is written as it is."""
    from camera_linearity_amd.measurand_factory import Measurand
    u8 = (family_image((64, 48), 3, seed=4).astype(np.int64) * top // 255).astype(np.uint8)
    u8[0, 0, 0] = top
    for how in ("constructor", "setter"):
        if how == "constructor":
            m = Measurand(torch.from_numpy(u8).to(DEV), None, True)
        else:
            m = Measurand(np.zeros(u8.shape), None, True)
            m.val = torch.from_numpy(u8).to(DEV)
        assert m.dn is not None and m._dn is None
        s = ImageSet(file_path=tmp_path / "10ms bf 5x frame.tif", measurand=m)
        s.save_8bit(tmp_path / "h.tif")
        s.save_8bit(tmp_path / "d.tif", device_encode=True)
        want, got = T.imread(tmp_path / "h.tif", T.IMREAD_UNCHANGED), T.imread(tmp_path / "d.tif", T.IMREAD_UNCHANGED)
        assert np.array_equal(got, want), how
        assert want.max() == (255 if top > 1 else 255 * top) and want.max() == got.max()
        if top == 199:
            assert not np.array_equal(want, u8)


# ---------------------------------------------------------------------------------------------------------------------
# 4. one writer, several sizes; 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_one_writer_for_a_large_a_small_and_a_large_image(tmp_path):
    w = T.DeviceTiffWriter(DEV)
    big, small = family_image((300, 257), 3, seed=5), family_image((3, 5), 3, seed=6)
    for k, img in enumerate((big, small, big[::-1].copy())):
        for compression in (5, 1):
            p = tmp_path / f"w{k}_{compression}.tif"
            T.imwrite_device(p, torch.from_numpy(img).to(DEV), compression=compression, predictor=2 if compression == 5 else 1, writer=w)
            T.imwrite(tmp_path / "host.tif", img, compression=compression, predictor=2 if compression == 5 else 1)
            assert p.read_bytes() == (tmp_path / "host.tif").read_bytes(), (k, compression)
    assert w.device == DEV


def test_imwrite_device_refuses_before_any_launch(tmp_path):
    calls = nat.hip_lib.calls["hm_tiff_encode_strips"]
    good = torch.zeros((8, 6, 3), dtype=torch.uint8, device=DEV)
    p = tmp_path / "no.tif"
    for t, kw in ((good.cpu(), {}), (good[:, ::2], {}), (good.transpose(0, 1), {}), (good.to(torch.float32), {}),
                  (good.to(torch.float64), dict(predictor=2)), (good, dict(compression=8)), (good, dict(quantize_divisor=2.0)),
                  (good.to(torch.float64), dict(quantize_divisor=0.0)), (good[:, :, :2].contiguous(), {})):
        with pytest.raises((ValueError, TypeError, NotImplementedError)):
            T.imwrite_device(p, t, **kw)
        assert not p.exists()
    assert nat.hip_lib.calls["hm_tiff_encode_strips"] == calls
