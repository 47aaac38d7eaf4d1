"""16-bit and float32 TIFF strips encoded on the MI355X (hm_tiff_encode_strips_wide through the raw C ABI, tiff_io.imwrite_device with
wide_samples / narrow_to_float32 / quantize_max_dn, ImageSet.save_32bit / save_16bit), against the host build's entry - which
tests/test_tiff_encode_wide_host.py pins against a NumPy expectation byte for byte on a box without a GPU - against NumPy directly for
the two conversions, and against tiff_io.imwrite's files. All inputs are valid."""
import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import tiff_io as T
from camera_linearity_amd.image_set import ImageSet

from test_tiff_device_host import bgr
from test_tiff_encode_wide_host import (F32, F64_AS_F32, F64_AS_U16, U16, abi_encode_wide, assert_narrowed, file_options, narrowing_vectors,
                                        odd_row, quantise_image_u16, source_image, strip_cases, wrap_image)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ENTRY = "hm_tiff_encode_strips_wide"


def assert_device_equals_host(name, img, kind, divisor, max_dn, rps, compression, predictor):
    want = abi_encode_wide(nat.host_lib(), img, kind, divisor, max_dn, rps, compression, predictor)
    got = abi_encode_wide(nat.hip_lib, img, kind, divisor, max_dn, rps, compression, predictor, on_device=True)
    assert want[3] == 0 and got[3] == 0, name
    assert np.array_equal(got[1], want[1]), f"{name}: offsets"
    assert np.array_equal(got[2], want[2]), f"{name}: counts"
    assert got[0].tobytes() == want[0].tobytes(), f"{name}: payload"
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. the C ABI against the host build
# ---------------------------------------------------------------------------------------------------------------------
def test_strip_family_is_byte_equal_to_the_host_build():
    """The cases of the host test: widths around the 64-lane step, 1 / 3 / 4 samples, the four kinds, both compressions, both
    predictors where they exist, a short last strip."""
    n = 0
    for name, img, kind, divisor, max_dn, rps, compression, predictor in strip_cases():
        assert_device_equals_host(name, img, kind, divisor, max_dn, rps, compression, predictor)
        n += 1
    assert n == 180


@pytest.mark.parametrize("samples", [1, 3, 4])
def test_predictor_wrap_rows(samples):
    img = wrap_image(samples)
    for compression in (1, 5):
        assert_device_equals_host(f"wrap s{samples} c{compression}", img, U16, 1.0, 0, 4, compression, 2)


# ---------------------------------------------------------------------------------------------------------------------
# 2. strip sizes at the LZW kernel's fetch and flush blocks
# ---------------------------------------------------------------------------------------------------------------------
def test_strips_around_the_fetch_and_flush_sizes():
    """The LZW kernel fetches 256 bytes at a time and flushes 64 words = 256 bytes; the wide pack kernel hands it strips of an even
    number of bytes. One-row grey uint16 strips of 254 .. 770 bytes: one sample below, at and above 256, 512 and 768."""
    rng = np.random.default_rng(3)
    for nbytes in (254, 256, 258, 510, 512, 514, 766, 768, 770):
        W = nbytes // 2
        for name, row in (("noise", rng.integers(0, 65536, W)), ("zeros", np.zeros(W)), ("ramp", np.arange(W) * 257 % 65536)):
            img = np.stack([row, row[::-1]]).astype(np.uint16)       # two strips
            assert_device_equals_host(f"{name}{nbytes}", img, U16, 1.0, 0, 1, 5, 1)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the grid-stride row loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compression", [1, 5])
def test_more_rows_than_the_pack_launch_has_waves(compression):
    """hm_tiff_encode_strips_wide launches the pack kernel on stream_grid(height * 64, 256, 8) workgroups: at most 8 per CU, each of 4
    waves with one row per wave. A height above CUs * 8 * 4 makes every wave take a second row."""
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    H = cus * 8 * 4 + 7
    img = (np.arange(H * 5, dtype=np.int64) * 7919 % 65521).astype(np.uint16).reshape(H, 5)
    _, offsets, counts, _ = assert_device_equals_host(f"{H} rows", img, U16, 1.0, 0, 1, compression, 2)
    if compression == 5:
        assert (counts > 0).all()
        assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(-(-counts // 16) * 16)]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. kinds 2 and 3 against NumPy
# ---------------------------------------------------------------------------------------------------------------------
def test_narrowing_on_the_device_is_astype_float32_bit_for_bit():
    """Float32 subnormal results included: the device units are built with float32 denormals on, and this is the test that says
    whether the conversion instruction honours it."""
    img, n_ties = narrowing_vectors()
    assert n_ties >= 700
    payload, _, _, rc = abi_encode_wide(nat.hip_lib, img, F64_AS_F32, 1.0, 0, 4, 1, 1, on_device=True)
    assert rc == 0
    assert_narrowed(payload.view("<u4"), img)


@pytest.mark.parametrize("max_dn", [511, 4095, 65535])
def test_quantisation_on_the_device_with_ties(max_dn):
    for d in (1.0, 3.7):
        img, n_ties = quantise_image_u16(d, max_dn)
        assert n_ties >= 200
        payload, _, _, rc = abi_encode_wide(nat.hip_lib, img, F64_AS_U16, d, max_dn, 4, 1, 1, on_device=True)
        assert rc == 0
        want = np.mod(np.around((img / d) * max_dn), 65536).astype(np.uint16)
        assert np.array_equal(payload.view("<u2").reshape(img.shape), bgr(want))
    odd, want = odd_row(max_dn)
    payload, _, _, rc = abi_encode_wide(nat.hip_lib, odd, F64_AS_U16, 1.0, max_dn, 1, 1, 1, on_device=True)
    assert rc == 0 and list(payload.view("<u2")) == want


# ---------------------------------------------------------------------------------------------------------------------
# 5. files
# ---------------------------------------------------------------------------------------------------------------------
def file_tensors():
    for W in (1, 65, 129):
        for samples in (1, 3, 4):
            yield f"u2s{samples}w{W}", source_image(U16, 70, W, samples, seed=W + samples)
        for samples in (1, 3):
            yield f"f4s{samples}w{W}", source_image(F32, 70, W, samples, seed=W + samples)


def test_device_files_are_byte_identical_to_imwrite_and_read_back(tmp_path):
    calls = nat.hip_lib.calls[ENTRY]
    n = 0
    for name, img in file_tensors():
        t = torch.from_numpy(img).to(DEV)
        for compression, predictor in file_options(img):
            T.imwrite(tmp_path / "host.tif", img, compression=compression, predictor=predictor, wide_samples=True)
            assert T.imwrite_device(tmp_path / "dev.tif", t, compression=compression, predictor=predictor, wide_samples=True)
            assert (tmp_path / "dev.tif").read_bytes() == (tmp_path / "host.tif").read_bytes(), (name, compression, predictor)
            back = T.imread_device(tmp_path / "dev.tif", T.IMREAD_UNCHANGED, device=DEV, wide_samples=True)
            assert back.dtype == t.dtype and back.shape == t.shape and torch.equal(back.view(torch.uint8), t.view(torch.uint8)), name
            n += 1
    assert n == 3 * (3 * 4 + 2 * 2) and nat.hip_lib.calls[ENTRY] == calls + n


def test_float64_tensors_as_float32_and_uint16_files(tmp_path):
    img, _ = narrowing_vectors()
    img = img[np.isfinite(img).all(axis=1)]                           # imread compares equal: no NaN rows
    for compression in (1, 5):
        p = tmp_path / "n.tif"
        T.imwrite_device(p, torch.from_numpy(img).to(DEV), compression=compression, narrow_to_float32=True)
        with np.errstate(over="ignore"):
            T.imwrite(tmp_path / "host.tif", img.astype(np.float32), compression=compression, wide_samples=True)
        assert p.read_bytes() == (tmp_path / "host.tif").read_bytes()
    for d, max_dn, compression, predictor in ((1.0, 4095, 1, 1), (3.7, 4095, 5, 2), (3.7, 65535, 1, 2), (1.0, 511, 5, 1)):
        img, _ = quantise_image_u16(d, max_dn)
        p = tmp_path / "q.tif"
        T.imwrite_device(p, torch.from_numpy(img).to(DEV), compression=compression, predictor=predictor, quantize_divisor=d,
                         quantize_max_dn=max_dn)
        got = T.imread(p, T.IMREAD_UNCHANGED)
        assert got.dtype == np.uint16 and np.array_equal(got, np.around((img / d) * max_dn).astype(np.uint16))
        lay = T._parse_layout(memoryview(p.read_bytes()))
        assert (lay.compression, lay.predictor) == (compression, predictor)


def test_one_writer_for_a_large_a_small_and_a_large_image(tmp_path):
    w = T.DeviceTiffWriter(DEV)
    big, small = source_image(U16, 300, 257, 3, seed=5), source_image(U16, 3, 5, 3, seed=6)
    for k, img in enumerate((big, small, big[::-1].copy())):
        for compression in (5, 1):
            p = tmp_path / f"w{k}_{compression}.tif"
            kw = dict(compression=compression, predictor=2 if compression == 5 else 1, wide_samples=True)
            T.imwrite_device(p, torch.from_numpy(img).to(DEV), writer=w, **kw)
            T.imwrite(tmp_path / "host.tif", img, **kw)
            assert p.read_bytes() == (tmp_path / "host.tif").read_bytes(), (k, compression)
    assert w.device == DEV


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_imwrite_device_wide_refuses_before_any_launch(tmp_path):
    calls = nat.hip_lib.calls[ENTRY], nat.hip_lib.calls["hm_tiff_encode_strips"]
    u16 = torch.zeros((8, 6, 3), dtype=torch.uint16, device=DEV)
    f32, f64 = torch.zeros((8, 6, 3), dtype=torch.float32, device=DEV), torch.zeros((8, 6, 3), dtype=torch.float64, device=DEV)
    wide = dict(wide_samples=True)
    p = tmp_path / "no.tif"
    for t, kw in ((u16, {}), (f32, {}), (u16, dict(compression=5)),                                   # without the keyword: as before
                  (u16.cpu(), wide), (u16[:, ::2], wide), (u16.transpose(0, 1), wide), (u16[:, :, :2].contiguous(), wide),
                  (u16, dict(wide, compression=8)), (u16, dict(wide, predictor=3)), (f32, dict(wide, predictor=2)),
                  (torch.zeros((8, 6, 3), dtype=torch.int16, device=DEV), wide), (torch.zeros((8, 6, 3), dtype=torch.float16, device=DEV), wide),
                  (u16, dict(wide, quantize_divisor=2.0)), (f32, dict(wide, quantize_max_dn=4095)), (u16, dict(wide, narrow_to_float32=True)),
                  (f32, dict(wide, narrow_to_float32=True)), (f64, dict(narrow_to_float32=True, predictor=2)),
                  (f64, dict(narrow_to_float32=True, quantize_max_dn=4095)), (f64, dict(narrow_to_float32=True, quantize_divisor=2.0)),
                  (f64, dict(quantize_max_dn=0)), (f64, dict(quantize_max_dn=65536)), (f64, dict(quantize_max_dn=4095.5)),
                  (f64, dict(quantize_max_dn=4095, quantize_divisor=0.0)), (f64, dict(quantize_max_dn=4095, compression=8))):
        with pytest.raises((ValueError, TypeError, NotImplementedError)):
            T.imwrite_device(p, t, **kw)
        assert not p.exists(), kw
    assert (nat.hip_lib.calls[ENTRY], nat.hip_lib.calls["hm_tiff_encode_strips"]) == calls


# ---------------------------------------------------------------------------------------------------------------------
# 7. ImageSet.save_32bit / save_16bit
# ---------------------------------------------------------------------------------------------------------------------
def merged_set(tmp_path, dtype):
    """A 64 x 48 x 3 'merged' image with values above 1 (so save_16bit scales) and a std image with values above 1 too."""
    rng = np.random.default_rng(33)
    val = rng.random((64, 48, 3)) * 5.0 + np.add.outer(np.arange(64), np.arange(48))[:, :, None] / 20.0
    std = rng.random((64, 48, 3)) * 1.5
    if dtype == torch.float64:
        return ImageSet(file_path=tmp_path / "10ms bf 5x merged.tif", value=val, std=std, use_cupy=True)
    from camera_linearity_amd.measurand_factory import Measurand
    m = Measurand(torch.from_numpy(val.astype(np.float32)).to(DEV), torch.from_numpy(std.astype(np.float32)).to(DEV), True)
    return ImageSet(file_path=tmp_path / "10ms bf 5x merged.tif", measurand=m)


def decoded(folder):
    return {p.name: T.imread(p, T.IMREAD_UNCHANGED) for p in sorted(folder.glob("*.tif"))}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("separate_channels", [False, True])
def test_save_32bit_device_encode(tmp_path, separate_channels, dtype):
    s = merged_set(tmp_path, dtype)
    assert s.measurand.val.dtype == dtype
    (tmp_path / "h").mkdir()
    (tmp_path / "d").mkdir()
    s.save_32bit(tmp_path / "h" / "m.tif", is_HDR=True, separate_channels=separate_channels)
    calls = nat.hip_lib.calls[ENTRY]
    s.save_32bit(tmp_path / "d" / "m.tif", is_HDR=True, separate_channels=separate_channels, device_encode=True)
    n_files = 6 if separate_channels else 2
    assert nat.hip_lib.calls[ENTRY] == calls + n_files
    names = sorted(p.name for p in (tmp_path / "h").glob("*.tif"))
    assert len(names) == n_files and names == sorted(p.name for p in (tmp_path / "d").glob("*.tif"))
    for name in names:
        assert (tmp_path / "d" / name).read_bytes() == (tmp_path / "h" / name).read_bytes(), name
        assert T.imread(tmp_path / "d" / name, T.IMREAD_UNCHANGED).dtype == np.float32


@pytest.mark.parametrize("force_16_bit,compression,predictor", [(False, 1, 1), (False, 5, 2), (True, 1, 2), (True, 5, 1)])
def test_save_16bit_device_encode(tmp_path, force_16_bit, compression, predictor):
    s = merged_set(tmp_path, torch.float64)
    (tmp_path / "h").mkdir()
    (tmp_path / "d").mkdir()
    kw = dict(bit_depth=12, force_16_bit=force_16_bit, compression=compression, predictor=predictor)
    s.save_16bit(tmp_path / "h" / "m.tif", **kw)
    calls = nat.hip_lib.calls[ENTRY]
    s.save_16bit(tmp_path / "d" / "m.tif", device_encode=True, **kw)
    assert nat.hip_lib.calls[ENTRY] == calls + (2 if force_16_bit else 1)
    got, want = decoded(tmp_path / "d"), decoded(tmp_path / "h")
    assert got.keys() == want.keys() and len(got) == 2
    for name in got:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    assert got["m.tif"].dtype == np.uint16 and got["m.tif"].max() == 4095
    assert got["m STD.tif"].dtype == (np.uint16 if force_16_bit else np.float64)
