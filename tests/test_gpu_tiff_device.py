"""TIFF strips decoded on the MI355X (hm_tiff_device.hip through tiff_io.imread_device and the raw C ABI), against the host path:
tiff_io.imread for whole files, hm_tiff_lzw_decode for single streams. Files and streams come from the encoder and writer of
tests/test_tiff_device_host.py, which checks them against the host decoders on a box without a GPU."""
import struct

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import tiff_io as T

import test_tiff_device_host as th
from test_tiff_device_host import bgr, family, family_image, host_lzw_decode, lzw_encode, pack_codes, write_tiff

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CANARY = 0xA5


def assert_same_as_imread(p, reader=None):
    for flag in (T.IMREAD_COLOR, T.IMREAD_UNCHANGED):
        want = T.imread(p, flag)
        got = T.imread_device(p, flag, device=DEV, reader=reader)
        assert isinstance(got, torch.Tensor) and got.device == DEV
        got = got.cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, (p.name, flag)
        assert np.array_equal(got, want), (p.name, flag)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the file family
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compression,predictor", [(1, 1), (1, 2), (5, 1), (5, 2)])
def test_file_family_is_byte_equal_to_imread(tmp_path, compression, predictor):
    """samples {1, 3, 4} x shape {(1, 1), (3, 5), (37, 101), (64, 64)} x rows per strip {1, 3, H, 2H}, both flags."""
    calls = nat.hip_lib.calls["hm_tiff_decode_strips"]
    n = 0
    for name, img, rps in family(compression, predictor):
        p = tmp_path / name
        write_tiff(p, img, rows_per_strip=rps, compression=compression, predictor=predictor)
        assert_same_as_imread(p)
        n += 2
    assert nat.hip_lib.calls["hm_tiff_decode_strips"] == calls + n


@pytest.mark.parametrize("compression", [1, 5])
def test_float64_files_are_byte_equal_to_imread(tmp_path, compression):
    """float64, 3 samples (and 1), IMREAD_UNCHANGED; first_offset 10 puts the strips off the 8-byte grid of the file (the byte path)."""
    rng = np.random.default_rng(3)
    for shape, rps, first in (((37, 23, 3), 1, 8), ((37, 23, 3), 5, 10), ((37, 23, 3), 37, 8), ((1, 1, 3), 1, 8), ((6, 7), 4, 8)):
        f = rng.random(shape)
        p = tmp_path / "f.tif"
        write_tiff(p, f, rows_per_strip=rps, compression=compression, first_offset=first)
        want = T.imread(p, T.IMREAD_UNCHANGED)
        got = T.imread_device(p, T.IMREAD_UNCHANGED, device=DEV).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)


def test_largest_image_single_strip_and_other_writers(tmp_path):
    """128 x 101 x 3 in ONE strip (38 KiB: past the 16 KiB a wave decodes in LDS, so the decoder works in place in the workspace), the
    same in one-row strips, imwrite's own files, a BigTIFF, a big-endian 8-bit file and - where Pillow is installed - libtiff's LZW."""
    img = family_image((128, 101), 3, seed=8)
    for rps in (128, 1, 50):
        p = tmp_path / f"big{rps}.tif"
        write_tiff(p, img, rows_per_strip=rps, compression=5, predictor=2)
        assert_same_as_imread(p)
    T.imwrite(tmp_path / "w8.tif", img)
    assert_same_as_imread(tmp_path / "w8.tif")
    f = np.random.default_rng(1).random((20, 31, 3))
    T.imwrite(tmp_path / "w64.tif", f)
    assert np.array_equal(T.imread_device(tmp_path / "w64.tif", T.IMREAD_UNCHANGED, device=DEV).cpu().numpy(), f)
    write_tiff(tmp_path / "mm.tif", img, rows_per_strip=3, compression=5, predictor=2, byteorder=">")
    assert_same_as_imread(tmp_path / "mm.tif")
    # BigTIFF, little-endian, 2 x 3 RGB float64 in one strip (the construction of test_tiff_io.test_big_endian_and_bigtiff)
    a = np.arange(18, dtype=np.float64).reshape(2, 3, 3) / 7
    data = a.tobytes()
    ents = [(256, 4, 1, 3), (257, 4, 1, 2), (258, 3, 3, None), (259, 3, 1, 1), (262, 3, 1, 2), (273, 4, 1, 16), (277, 3, 1, 3),
            (278, 4, 1, 2), (279, 4, 1, len(data)), (339, 3, 3, None)]
    ifd = struct.pack("<Q", len(ents))
    for tag, typ, cnt, val in ents:
        if val is None:
            ifd += struct.pack("<HHQ", tag, typ, cnt) + struct.pack("<HHH", *([64] * 3 if tag == 258 else [3] * 3)).ljust(8, b"\0")
        else:
            ifd += struct.pack("<HHQ", tag, typ, cnt) + struct.pack("<H" if typ == 3 else "<I", val).ljust(8, b"\0")
    ifd += struct.pack("<Q", 0)
    (tmp_path / "big.tif").write_bytes(struct.pack("<2sHHHQ", b"II", 43, 8, 0, 16 + len(data)) + data + ifd)
    assert np.array_equal(T.imread_device(tmp_path / "big.tif", T.IMREAD_UNCHANGED, device=DEV).cpu().numpy(), a[:, :, ::-1])
    Image = pytest.importorskip("PIL.Image")
    Image.fromarray(img).save(tmp_path / "pil.tif", format="TIFF", compression="tiff_lzw", tiffinfo={317: 2, 278: 3})
    assert_same_as_imread(tmp_path / "pil.tif")


# ---------------------------------------------------------------------------------------------------------------------
# the raw ABI: strips of one byte per pixel, one row per strip, with canaries round everything the call writes
# ---------------------------------------------------------------------------------------------------------------------
def guarded(n_bytes, fill=0):
    buf = torch.full((64 + n_bytes + 64,), CANARY, dtype=torch.uint8, device=DEV)
    buf[64:64 + n_bytes] = fill
    return buf


def canaries_intact(buf, n_bytes):
    h = buf.cpu().numpy()
    return bool((h[:64] == CANARY).all() and (h[64 + n_bytes:] == CANARY).all())


def decode_rows(streams, width, offsets=None, counts=None, file_len=None):
    """One launch: strip s = streams[s], one row of `width` one-byte pixels each. Returns (status, dst rows, canaries intact).
    `offsets` / `counts` / `file_len` override what is told about the file (for the out-of-range strip)."""
    n = len(streams)
    blob = b"".join(streams)
    offs = np.cumsum([0] + [len(s) for s in streams[:-1]]).astype(np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)
    cnts = np.array([len(s) for s in streams], dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64)
    file_len = len(blob) if file_len is None else file_len
    file = torch.as_tensor(np.frombuffer(blob + bytes(8), dtype=np.uint8).copy(), device=DEV)
    tables = torch.as_tensor(np.concatenate([offs, cnts]), device=DEV)
    ws_bytes = nat.hip_lib.hm_tiff_decode_workspace_bytes(n, width, 5)
    assert ws_bytes == n * width
    dst, status, ws = guarded(n * width, fill=0xEE), guarded(8 * n), guarded(ws_bytes)
    rc = nat.hip_lib.hm_tiff_decode_strips(file.data_ptr(), file_len, tables.data_ptr(), tables.data_ptr() + 8 * n, n, 5, 1, 1, n, width,
                                           1, 1, 0, dst.data_ptr() + 64, status.data_ptr() + 64, ws.data_ptr() + 64,
                                           nat.current_stream_ptr(DEV))
    assert rc == nat.HM_OK
    torch.cuda.synchronize(DEV)
    st = status[64:64 + 8 * n].cpu().numpy().view(np.int64)
    rows = dst[64:64 + n * width].cpu().numpy().reshape(n, width)
    ok = canaries_intact(dst, n * width) and canaries_intact(status, 8 * n) and canaries_intact(ws, ws_bytes)
    return st, rows, ok


def long_cases():
    """Strips past the 16 KiB the decoder stages in LDS: the same features decoded in place in global memory."""
    rng = np.random.default_rng(12)
    noise = rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()
    constant = bytes([7]) * 20000
    return {"noise_long": (noise, lzw_encode(noise)), "constant_long": (constant, lzw_encode(constant))}


@pytest.mark.parametrize("name", ["noise", "constant", "periodic", "no_eoi", "hand", "noise_long", "constant_long"])
def test_stream_features_match_the_host_decoder(name):
    """noise: >= 11 KiB, the table fills, a mid-strip Clear, every width 9..12; constant: every code KwKwK, strings longer than a wave;
    periodic; no EOI; the hand-assembled Clear 'A' 'B' 258 260 EOI. Bytes and return value are hm_tiff_lzw_decode's."""
    plain, stream = {**th.stream_cases(), **long_cases()}[name]
    want_n, want = host_lzw_decode(stream, len(plain))
    assert want_n == len(plain) and want == plain
    st, rows, ok = decode_rows([stream], len(plain))
    assert st[0] == want_n
    assert rows[0].tobytes() == want
    assert ok


def test_status_and_isolation():
    """8 strips in one launch: one whose stream outgrows its row (HM_ESHAPE), one with an invalid code (HM_EINVAL), one whose range ends
    past the file (rejected without a read); the other five decode, the bad ones leave their rows alone, the canaries stand."""
    W = 300
    rng = np.random.default_rng(21)
    plains = [rng.integers(0, 256 if s % 2 else 8, W, dtype=np.uint8).tobytes() for s in range(8)]
    streams = [lzw_encode(p) for p in plains]
    streams[2] = lzw_encode(plains[2] + b"xy")                        # 302 bytes into a row of 300
    streams[4] = pack_codes([256, 65, 300, 257])                      # 300 > next (259)
    offs = np.cumsum([0] + [len(s) for s in streams[:-1]])
    cnts = np.array([len(s) for s in streams])
    file_len = int(offs[-1] + cnts[-1])
    offs[6], cnts[6] = file_len - 10, 100                             # ends 90 bytes past the file
    assert host_lzw_decode(streams[2], W)[0] == nat.HM_ESHAPE and host_lzw_decode(streams[4], W)[0] == nat.HM_EINVAL
    st, rows, ok = decode_rows(streams, W, offsets=offs, counts=cnts, file_len=file_len)
    assert list(st) == [W, W, nat.HM_ESHAPE, W, nat.HM_EINVAL, W, nat.HM_EINVAL, W]
    for s in (0, 1, 3, 5, 7):
        assert rows[s].tobytes() == plains[s], s
    for s in (2, 4, 6):
        assert (rows[s] == 0xEE).all(), s
    assert ok
    # the same out-of-range strip in an uncompressed file: the only kernel of that path refuses it too
    n = 4
    file = torch.as_tensor(np.arange(4 * 16, dtype=np.uint8), device=DEV)
    tables = torch.as_tensor(np.array([0, 16, 60, 48, 16, 16, 16, 16], dtype=np.int64), device=DEV)
    dst, status = guarded(n * 16, fill=0xEE), guarded(8 * n)
    assert nat.hip_lib.hm_tiff_decode_strips(file.data_ptr(), 64, tables.data_ptr(), tables.data_ptr() + 8 * n, n, 1, 1, 1, n, 16, 1, 1, 0,
                                             dst.data_ptr() + 64, status.data_ptr() + 64, None, nat.current_stream_ptr(DEV)) == nat.HM_OK
    torch.cuda.synchronize(DEV)
    assert list(status[64:64 + 8 * n].cpu().numpy().view(np.int64)) == [16, 16, nat.HM_EINVAL, 16]
    rows = dst[64:64 + 64].cpu().numpy().reshape(4, 16)
    assert np.array_equal(rows[[0, 1, 3]], np.arange(64, dtype=np.uint8).reshape(4, 16)[[0, 1, 3]]) and (rows[2] == 0xEE).all()
    assert canaries_intact(dst, 64) and canaries_intact(status, 32)


CORRUPT_SEED = 0          # chosen on the host (corrupted_strips needs no GPU): the host decoder refuses 32 of the 64 strips and decodes 32
CORRUPT_WIDTH = 600


def corrupted_strips(seed=CORRUPT_SEED, width=CORRUPT_WIDTH):
    """64 strips from valid streams of `width` bytes (noise, few-valued, constant, periodic) by seeded bit flips and truncations."""
    rng = np.random.default_rng(seed)
    bases = [rng.integers(0, 256, width, dtype=np.uint8).tobytes(), rng.integers(0, 4, width, dtype=np.uint8).tobytes(),
             bytes([9]) * width, bytes([1, 2, 3]) * (width // 3)]
    out = []
    for k in range(64):
        b = bytearray(lzw_encode(bases[k % 4]))
        if k % 3 == 2:
            b = b[:int(rng.integers(1, len(b)))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(b))
    return out


def test_fixed_corrupted_set_reports_what_the_host_reports():
    """Error reporting on a fixed set, once: for each of 64 damaged strips the device status is the host decoder's return value, and
    where that is not negative the bytes are the host's."""
    streams = corrupted_strips()
    host = [host_lzw_decode(s, CORRUPT_WIDTH) for s in streams]
    assert sum(n < 0 for n, _ in host) >= 16 and sum(n >= 0 for n, _ in host) >= 16
    assert {n for n, _ in host if n < 0} == {nat.HM_EINVAL, nat.HM_ESHAPE}
    st, rows, ok = decode_rows(streams, CORRUPT_WIDTH)
    assert list(st) == [n for n, _ in host]
    for s, (n, data) in enumerate(host):
        if n >= 0:
            assert rows[s, :n].tobytes() == data, s
    assert ok


# ---------------------------------------------------------------------------------------------------------------------
# 5. the workflow, 6. one reader for many files
# ---------------------------------------------------------------------------------------------------------------------
def test_workflow_is_bit_equal_to_the_host_decode(tmp_path):
    from camera_linearity_amd.exposure_series import ExposureSeries
    from oracle import hdr_oracle as orc
    rng = np.random.default_rng(31)
    scene = rng.random((64, 48, 3)) * 0.9 + 0.05
    for ms in (10, 20, 40):
        dn = np.clip(np.around(scene * ms / 40 * 255 + rng.normal(0, 1, scene.shape)), 0, 255).astype(np.uint8)
        write_tiff(tmp_path / f"{ms}ms bf 5x scene.tif", dn, rows_per_strip=7, compression=5, predictor=2)
        write_tiff(tmp_path / f"{ms}ms bf 5x scene STD.tif", 0.002 + 0.01 * rng.random(scene.shape), rows_per_strip=5, compression=5)
    icrf, diff = orc.synthetic_icrf()

    def run(device_decode):
        (series,) = ExposureSeries.from_dir_path(tmp_path, use_cupy=True)
        series.load_value_images(device_decode=device_decode)
        series.load_std_images(device_decode=device_decode)
        series.process_HDR_image(icrf, diff)
        return series.merged_image_set.host_arrays()

    val0, std0 = run(False)
    before = dict(nat.hip_lib.calls)
    val1, std1 = run(True)
    assert nat.hip_lib.calls["hm_tiff_decode_strips"] == before.get("hm_tiff_decode_strips", 0) + 6
    assert nat.hip_lib.calls["hm_tiff_lzw_decode"] == before["hm_tiff_lzw_decode"] > 0
    assert val0.shape == (64, 48, 3) and std0 is not None and std1 is not None
    assert np.array_equal(val0.view(np.uint64), val1.view(np.uint64))
    assert np.array_equal(std0.view(np.uint64), std1.view(np.uint64))


def test_one_reader_large_small_large(tmp_path):
    """Stale bytes of a longer file (its data, its strip tables, its statuses, its workspace) do not leak into a shorter one."""
    big = family_image((128, 101), 3, seed=41)
    small = family_image((3, 5), 3, seed=42)
    write_tiff(tmp_path / "big.tif", big, rows_per_strip=1, compression=5, predictor=2)
    write_tiff(tmp_path / "small.tif", small, rows_per_strip=2, compression=5, predictor=2)
    write_tiff(tmp_path / "small_raw.tif", small[:, :, 0], rows_per_strip=3)
    reader = T.DeviceTiffReader(DEV)
    first = reader.read(tmp_path / "big.tif", T.IMREAD_UNCHANGED).cpu().numpy()
    assert np.array_equal(first, bgr(big))
    for name in ("small.tif", "big.tif", "small_raw.tif", "small.tif", "big.tif"):
        assert_same_as_imread(tmp_path / name, reader=reader)
    assert reader.read(tmp_path / "absent.tif") is None
    # a damaged strip is named, and the reader goes on working
    raw = bytearray((tmp_path / "big.tif").read_bytes())
    lay = T._parse_layout(memoryview(bytes(raw)))
    raw[lay.offsets[5]:lay.offsets[5] + 3] = pack_codes([256, 300])[:3]
    (tmp_path / "bad.tif").write_bytes(bytes(raw))
    with pytest.raises(T.TiffError, match="strip 5"):
        reader.read(tmp_path / "bad.tif")
    with pytest.raises(T.TiffError):
        T.imread(tmp_path / "bad.tif")
    assert_same_as_imread(tmp_path / "big.tif", reader=reader)
