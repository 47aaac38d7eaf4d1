"""uint16, float32 and big-endian TIFF strips decoded on the MI355X (hm_tiff_decode_strips_wide through
tiff_io.imread_device(wide_samples=True) and the raw C ABI), against the host path: tiff_io.imread for whole files, the host build's
entry for status words and partial rows. Files and fixed damaged inputs come from tests/test_tiff_device_wide_host.py, which checks
them against the host decoders on a box without a GPU."""
import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import tiff_io as T

import test_tiff_device_wide_host as wh
from test_tiff_device_host import family_image, write_tiff

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TORCH_DTYPES = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.float32): torch.float32,
                np.dtype(np.float64): torch.float64}


def host_bytes(t):
    """A device tensor's bytes on the host (uint16 tensors travel as bytes: nothing here depends on torch's uint16 operators)."""
    return t.contiguous().view(torch.uint8).cpu().numpy()


def assert_same_as_imread(p, flags, reader=None):
    for flag in flags:
        want = T.imread(p, flag)
        got = T.imread_device(p, flag, device=DEV, reader=reader, wide_samples=True)
        assert isinstance(got, torch.Tensor) and got.device == DEV
        assert got.dtype == TORCH_DTYPES[want.dtype] and tuple(got.shape) == want.shape, (p.name, flag)
        assert host_bytes(got).tobytes() == want.tobytes(), (p.name, flag)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the file family
# ---------------------------------------------------------------------------------------------------------------------
def check_family(tmp_path, dtype, compression, predictor, byteorder):
    calls = nat.hip_lib.calls["hm_tiff_decode_strips_wide"]
    n = 0
    for name, img, kw in wh.wide_family(dtype, compression, predictor, byteorder):
        p = tmp_path / name
        write_tiff(p, img, **kw)
        assert_same_as_imread(p, wh.flags_of(dtype))
        n += len(wh.flags_of(dtype))
    assert nat.hip_lib.calls["hm_tiff_decode_strips_wide"] == calls + n


@pytest.mark.parametrize("compression,predictor,byteorder", wh.U16_KINDS)
def test_uint16_family_is_byte_equal_to_imread(tmp_path, compression, predictor, byteorder):
    """samples {1, 3, 4} x widths {1, 47, 63, 64, 65, 129} and one 3000-pixel row x rows per strip {1, 3, H}, both flags; uncompressed
    files also with every strip at an odd offset."""
    check_family(tmp_path, np.uint16, compression, predictor, byteorder)


@pytest.mark.parametrize("dtype,compression,byteorder", wh.FLOAT_KINDS)
def test_float_family_is_byte_equal_to_imread(tmp_path, dtype, compression, byteorder):
    """float32 in either byte order and big-endian float64, 1 / 3 samples, IMREAD_UNCHANGED: bit patterns, not values, are compared."""
    check_family(tmp_path, dtype, compression, 1, byteorder)


def test_one_reader_large_small_large(tmp_path):
    """Stale bytes of a longer file do not leak into a shorter one, across sample types, through one reader's buffers."""
    big = wh.wide_image((40, 129), 3, seed=41)
    small = wh.wide_image((3, 5), 3, seed=42)
    f32 = wh.float_image((3, 5), 1, np.float32, seed=43)
    write_tiff(tmp_path / "big.tif", big, rows_per_strip=1, compression=5, predictor=2, byteorder=">")
    write_tiff(tmp_path / "small.tif", small, rows_per_strip=2, compression=5, predictor=2)
    write_tiff(tmp_path / "small_f32.tif", f32, rows_per_strip=3, first_offset=9)
    u8 = family_image((3, 5), 3, seed=44)
    write_tiff(tmp_path / "small_u8.tif", u8, compression=5, predictor=2)
    reader = T.DeviceTiffReader(DEV)
    both = (T.IMREAD_COLOR, T.IMREAD_UNCHANGED)
    for name, flags in (("big.tif", both), ("small.tif", both), ("big.tif", both), ("small_f32.tif", both[1:]), ("small_u8.tif", both),
                        ("big.tif", both)):
        assert_same_as_imread(tmp_path / name, flags, reader=reader)
    assert reader.read(tmp_path / "absent.tif", T.IMREAD_UNCHANGED, wide_samples=True) is None


def test_wide_samples_is_opt_in(tmp_path):
    """Without the keyword a uint16 file is refused as before (this holds before and after the wide entry: a guard, not its proof)."""
    write_tiff(tmp_path / "u16.tif", wh.wide_image((4, 5), 3, seed=1))
    with pytest.raises(NotImplementedError, match=r"tiff_io\.imread"):
        T.imread_device(tmp_path / "u16.tif", T.IMREAD_UNCHANGED, device=DEV)
    with pytest.raises(NotImplementedError, match=r"tiff_io\.imread"):
        T.DeviceTiffReader(DEV).read(tmp_path / "u16.tif", T.IMREAD_COLOR)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the raw ABI on guarded device buffers: fixed inputs the decoder refuses or cuts short by design, against the host build
# ---------------------------------------------------------------------------------------------------------------------
def guarded(n_bytes, fill):
    buf = torch.full((64 + n_bytes + 64,), wh.CANARY, dtype=torch.uint8, device=DEV)
    buf[64:64 + n_bytes] = fill
    return buf


def canaries_intact(buf, n_bytes):
    h = buf.cpu().numpy()
    return bool((h[:64] == wh.CANARY).all() and (h[64 + n_bytes:] == wh.CANARY).all())


def device_wide_call(case):
    """wh.host_wide_call on device buffers with canaries round everything the call writes: (status, rows, canaries intact)."""
    n = case["H"]
    file = torch.as_tensor(np.frombuffer(case["blob"] + bytes(8), dtype=np.uint8).copy(), device=DEV)
    tables = torch.as_tensor(np.concatenate([np.asarray(case["offs"], dtype=np.int64), np.asarray(case["cnts"], dtype=np.int64)]), device=DEV)
    rb = wh.out_row_bytes(case)
    ws_bytes = nat.hip_lib.hm_tiff_decode_workspace_bytes(n, case["W"] * case["S"] * case["bps"], case["comp"])
    dst, status, ws = guarded(n * rb, wh.FILL), guarded(8 * n, 0), guarded(ws_bytes, 0)
    rc = nat.hip_lib.hm_tiff_decode_strips_wide(file.data_ptr(), case["file_len"], tables.data_ptr(), tables.data_ptr() + 8 * n, n,
                                                case["comp"], case["pred"], 1, n, case["W"], case["S"], case["bps"], case["be"],
                                                case["color"], dst.data_ptr() + 64, status.data_ptr() + 64, ws.data_ptr() + 64,
                                                nat.current_stream_ptr(DEV))
    assert rc == nat.HM_OK
    torch.cuda.synchronize(DEV)
    st = status[64:64 + 8 * n].cpu().numpy().view(np.int64)
    rows = dst[64:64 + n * rb].cpu().numpy().reshape(n, rb)
    ok = canaries_intact(dst, n * rb) and canaries_intact(status, 8 * n) and canaries_intact(ws, ws_bytes)
    return st, rows, ok


@pytest.mark.parametrize("name", sorted(wh.damaged_cases()))
def test_status_isolation_and_canaries_match_the_host_build(name):
    """Short strips (counts that end 1, 3, 5 and 7 bytes into a pixel), an LZW strip with an invalid code and strips beyond the end of
    the file: the device's status words and every byte of dst - decoded, partly decoded and untouched rows - are the host build's, and
    nothing outside dst, the status and the workspace is written."""
    case = wh.damaged_cases()[name]
    want_st, want_rows, host_ok = wh.host_wide_call(nat.host_lib(), case)
    assert host_ok
    st, rows, ok = device_wide_call(case)
    assert list(st) == list(want_st)
    assert np.array_equal(rows, want_rows)
    assert (st < 0).any() or (rows == wh.FILL).any()                  # the case did leave something out
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 3. the workflow
# ---------------------------------------------------------------------------------------------------------------------
def test_uint16_frames_merge_bit_equal_through_both_decoders(tmp_path):
    """Three 12-bit frames as 16-bit LZW + Predictor 2 files: imread + upload and imread_device give the same uint16 tensors, and
    engine.merge(bit_depth=12) of the two gives the same bits."""
    from camera_linearity_amd import engine
    rng = np.random.default_rng(51)
    scene = rng.random((9, 70, 3)) * 0.9 + 0.05
    exposures = [1e-3, 2e-3, 4e-3]
    icrf = np.stack([np.linspace(0, 1, 4096) ** 1.1] * 3, axis=1)
    host, dev = [], []
    for i, t in enumerate(exposures):
        dn = np.clip(np.around(scene * t / 4e-3 * 4095 + rng.normal(0, 3, scene.shape)), 0, 4095).astype(np.uint16)
        p = tmp_path / f"f{i}.tif"
        write_tiff(p, dn[:, :, ::-1], rows_per_strip=2, compression=5, predictor=2)
        a = T.imread(p, T.IMREAD_UNCHANGED)
        assert a.dtype == np.uint16 and np.array_equal(a, dn)
        host.append(torch.as_tensor(a, device=DEV))
        dev.append(T.imread_device(p, T.IMREAD_UNCHANGED, device=DEV, wide_samples=True))
        assert dev[-1].dtype == torch.uint16 and host_bytes(dev[-1]).tobytes() == host_bytes(host[-1]).tobytes()
    want = engine.merge(host, exposures, icrf, bit_depth=12)["val"]
    got = engine.merge(dev, exposures, icrf, bit_depth=12)["val"]
    torch.cuda.synchronize(DEV)
    assert want.dtype == torch.float64 and torch.isfinite(want).all()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want.cpu().numpy().view(np.uint64))


def _features(t):
    return {"illumination": "bf", "magnification": "5x", "exposure": float(t), "subject": "scene"}


def test_float32_std_files_workflow_is_bit_equal_to_the_host_decode(tmp_path):
    """An 8-bit series with the float32 ' STD.tif' files save_32bit writes: device_decode=True gives measurand.std the same float32
    bits as the default path, and process_HDR_image the same outputs."""
    from camera_linearity_amd.exposure_series import ExposureSeries
    from camera_linearity_amd.image_set import ImageSet
    from oracle import hdr_oracle as orc
    rng = np.random.default_rng(52)
    scene = rng.random((9, 70, 3)) * 0.9 + 0.05
    for ms in (10, 20, 40):
        dn = np.clip(np.around(scene * ms / 40 * 255 + rng.normal(0, 1, scene.shape)), 0, 255).astype(np.uint8)
        sd = (0.002 + 0.01 * rng.random(scene.shape)).astype(np.float32)
        path = tmp_path / f"{ms}ms bf 5x scene.tif"
        ImageSet(value=dn, std=sd, features=_features(ms / 1000), use_cupy=False).save_32bit(save_path=path)
        write_tiff(path, dn[:, :, ::-1], rows_per_strip=4, compression=5, predictor=2)     # the DNs under the value image's name
        assert T.imread(tmp_path / f"{ms}ms bf 5x scene STD.tif", T.IMREAD_UNCHANGED).dtype == np.float32
    icrf, diff = orc.synthetic_icrf()

    def run(device_decode):
        (series,) = ExposureSeries.from_dir_path(tmp_path, use_cupy=True)
        series.load_value_images(device_decode=device_decode)
        series.load_std_images(device_decode=device_decode)
        stds = [s.measurand._std for s in series.input_image_sets]
        series.process_HDR_image(icrf, diff)
        return stds, series.merged_image_set.host_arrays()

    stds0, (val0, std0) = run(False)
    before = nat.hip_lib.calls["hm_tiff_decode_strips_wide"]
    stds1, (val1, std1) = run(True)
    assert nat.hip_lib.calls["hm_tiff_decode_strips_wide"] == before + 3
    for a, b in zip(stds0, stds1):
        assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    assert std0 is not None and std1 is not None and val0.shape == (9, 70, 3)
    assert np.array_equal(val0.view(np.uint64), val1.view(np.uint64))
    assert np.array_equal(std0.view(np.uint64), std1.view(np.uint64))


def test_uint16_value_file_loads_like_the_default_path(tmp_path):
    """A 16-bit value file through ImageSet.load_value_image(device_decode=True): `>> 8` as uint8 DNs, or float64 with bit64."""
    from camera_linearity_amd.image_set import ImageSet
    img = wh.wide_image((9, 70), 3, seed=53)
    p = tmp_path / "10ms bf 5x scene.tif"
    write_tiff(p, img, rows_per_strip=4, compression=5, predictor=2, byteorder=">")
    for bit64 in (False, True):
        a, b = ImageSet(file_path=p, use_cupy=True), ImageSet(file_path=p, use_cupy=True)
        a.load_value_image(bit64=bit64)
        b.load_value_image(bit64=bit64, device_decode=True)
        va, vb = a.host_arrays()[0], b.host_arrays()[0]
        assert va.dtype == vb.dtype == np.float64 and np.array_equal(va.view(np.uint64), vb.view(np.uint64))
