"""TIFF reading / writing with OpenCV's conventions, without OpenCV.

The reference moves every image through `cv.imread` / `cv.imwrite` (modules/image_set.py:214-243, 264-363;
modules/video_processing.py:236): 8-bit BGR TIFFs for acquired frames, float64 three-channel TIFFs for the
` STD.tif` / ` HDR.tif` companions. OpenCV is not available here, so this module is a small codec for exactly
that family of files:

  read   classic and BigTIFF, either byte order, strips (not tiles), chunky planar configuration,
         1/3/4 samples of uint8 / uint16 / float32 / float64, Compression none (1), LZW (5, with libtiff's early
         change), Deflate (8 / 32946), PackBits (32773), Predictor 1 / 2 (horizontal differencing)
  write  classic TIFF (BigTIFF when the file would pass 4 GiB), one strip per ~8 KiB of rows like OpenCV,
         uint8 / uint16 / float32 / float64 uncompressed (the default); on request LZW (5, what cv.imwrite's TIFF writer
         uses) for uint8 / float64 and Predictor 2 for uint8, encoded by the host build's hm_tiff_encode_strips; with
         `wide_samples=True` also LZW for uint16 / float32 and Predictor 2 for uint16 (hm_tiff_encode_strips_wide) - the layout
         camera software and cv.imwrite give 9- to 16-bit frames

`imread` / `imwrite` follow OpenCV's channel convention: files hold RGB(A), arrays are BGR(A). OpenCV applies
the swap on both sides for every depth, so a file written here and read by the reference (or the reverse) shows
the same channel order.  `imread(path)` (no flag) returns 8-bit BGR like `cv.imread(path)`,
`imread(path, IMREAD_UNCHANGED)` returns the stored dtype like `cv.imread(path, cv.IMREAD_UNCHANGED)`.

Parity note: the reference holds no TIFF fixtures and cv2 is absent, so interoperability is checked against
Pillow/libtiff (tests/test_tiff_io.py) for the integer formats; the float64 three-channel layout (SampleFormat 3,
BitsPerSample 64,64,64, RGB order in the file) follows the TIFF 6.0 specification and is parity-unpinned against cv2.

The byte-serial LZW / PackBits loops run in libhdrmerge.so's host code (hm_tiff_lzw_decode); strips are decoded
on a thread pool. That is `imread`, the default path, and it reads the whole family above.

`imread_device` is the opt-in device path for the files of the documented workflow (8-bit frames, float64 companions):
the file's bytes are uploaded as they are and hm_tiff_decode_strips (csrc/hm_tiff_device.hip) decodes the LZW strips, undoes
Predictor 2, swaps R and B and applies the imread flag on the GPU, so the frame is born in device memory. It reads
little-endian samples of uint8 (1 / 3 / 4 samples, Predictor 1 / 2) and float64 (1 / 3 samples), Compression 1 and 5,
strips, chunky; everything else it refuses with NotImplementedError - there is no fallback, `imread` is the host path.
A `DeviceTiffReader` owns the staging and device buffers and is reused across the files of a series.
`imread_device(..., wide_samples=True)` widens that family through hm_tiff_decode_strips_wide: uint16 (1 / 3 / 4 samples,
Predictor 1 / 2, both flags - the DN frames of 9- to 16-bit cameras), float32 and float64 (1 / 3 samples, IMREAD_UNCHANGED), in
either byte order. Without the keyword every refusal stays as it was.

`imwrite_device` is its writing twin: a uint8 or float64 tensor in device memory goes through hm_tiff_encode_strips
(csrc/hm_tiff_encode.hip) - optional quantisation to uint8, R/B swap, Predictor 2, LZW, compaction - and comes down as one payload
that is written between the header and the IFD. Compression 1 gives the very bytes `imwrite` writes. A `DeviceTiffWriter` owns
the buffers. `imwrite_device(..., wide_samples=True)` widens that family through hm_tiff_encode_strips_wide: torch.uint16 tensors
(Predictor 1 / 2) and torch.float32 tensors (bit for bit), Compression 1 and 5; a float64 tensor is stored as float32 with
`narrow_to_float32=True` (the rounding of ndarray.astype(np.float32)) and as uint16 with `quantize_divisor=d, quantize_max_dn=m`
(around((v / d) * m), save_16bit's arithmetic). Without these keywords every refusal stays as it was. Not written on the device:
tiles, Deflate, PackBits, big-endian files, Predictor 2 or 3 on float samples; there is no fallback, `imwrite` is the host path.
"""
from __future__ import annotations

import ctypes as C
import mmap
import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

IMREAD_UNCHANGED = -1          # cv.IMREAD_UNCHANGED
IMREAD_COLOR = 1               # cv.IMREAD_COLOR (the default of cv.imread)

_TYPE_SIZES = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 16: 8, 17: 8, 18: 8}
_TYPE_FMT = {1: "B", 2: "c", 3: "H", 4: "I", 6: "b", 7: "B", 8: "h", 9: "i", 11: "f", 12: "d", 16: "Q", 17: "q", 18: "Q"}


class TiffError(ValueError):
    pass


def _native():
    from . import _native as nat          # deferred: only compressed strips need the library
    return nat


def _read_ifd(buf: memoryview, bo: str, big: bool, off: int):
    tags = {}
    if big:
        (n,) = struct.unpack_from(bo + "Q", buf, off)
        pos, esz, inline = off + 8, 20, 8
    else:
        (n,) = struct.unpack_from(bo + "H", buf, off)
        pos, esz, inline = off + 2, 12, 4
    for i in range(n):
        e = pos + i * esz
        tag, typ = struct.unpack_from(bo + "HH", buf, e)
        (cnt,) = struct.unpack_from(bo + ("Q" if big else "I"), buf, e + 4)
        voff = e + (12 if big else 8)
        size = _TYPE_SIZES.get(typ)
        if size is None:
            continue
        if size * cnt > len(buf):
            raise TiffError(f"TIFF tag {tag} claims {cnt} values, more than the file holds")
        if size * cnt > inline:
            (voff,) = struct.unpack_from(bo + ("Q" if big else "I"), buf, voff)
        if typ in (5, 10):
            raw = struct.unpack_from(bo + ("I" if typ == 5 else "i") * (2 * cnt), buf, voff)
            tags[tag] = tuple(raw[2 * k] / raw[2 * k + 1] if raw[2 * k + 1] else 0.0 for k in range(cnt))
        elif typ == 2:
            tags[tag] = bytes(buf[voff:voff + cnt])
        else:
            tags[tag] = struct.unpack_from(bo + _TYPE_FMT[typ] * cnt, buf, voff)
    return tags


def _decode_strip(data: bytes, compression: int, expected: int) -> bytes:
    if compression == 1:
        return data
    if compression in (8, 32946):
        return zlib.decompress(data)
    if compression in (5, 32773):
        nat = _native()
        out = (C.c_uint8 * expected)()
        fn = nat.lib.hm_tiff_lzw_decode if compression == 5 else nat.lib.hm_tiff_packbits_decode
        n = fn(data, len(data), out, expected)
        if n < 0:
            raise TiffError(f"corrupt {'LZW' if compression == 5 else 'PackBits'} strip ({nat.strerror(int(n))})")
        return bytes(memoryview(out)[:n])
    raise NotImplementedError(f"TIFF compression {compression} is not supported")


def read_tiff(path) -> np.ndarray:
    """First image of a TIFF file as stored: (H, W) or (H, W, S) in FILE sample order (RGB), file dtype.
    Malformed files raise TiffError (a ValueError)."""
    with open(path, "rb") as f:
        buf = memoryview(f.read())
    try:
        return _read_tiff(buf)
    except (struct.error, IndexError, zlib.error, OverflowError, MemoryError) as e:
        raise TiffError(f"malformed TIFF file {path}: {e}") from e


class TiffLayout(NamedTuple):
    """What the first IFD says about the pixels: everything a decoder needs, nothing decoded yet."""
    dtype: np.dtype            # of a sample, in the FILE's byte order
    shape: Tuple[int, int, int]   # (H, W, samples per pixel)
    rows_per_strip: int        # clamped to 1..H
    offsets: Sequence[int]     # StripOffsets, at least n_strips of them
    counts: Sequence[int]      # StripByteCounts (derived for uncompressed files that lack them)
    compression: int
    predictor: int
    photometric: int

    @property
    def n_strips(self) -> int:
        return (self.shape[0] + self.rows_per_strip - 1) // self.rows_per_strip

    @property
    def row_bytes(self) -> int:
        return self.shape[1] * self.shape[2] * self.dtype.itemsize


def _parse_layout(buf: memoryview) -> TiffLayout:
    """Header and first IFD of a TIFF file -> TiffLayout. Raises what _read_tiff raises for a file it cannot lay out
    (TiffError, NotImplementedError for tiles / mixed depths / planar samples / unknown sample formats)."""
    if len(buf) < 8:
        raise TiffError("not a TIFF file (too short)")
    bo = {b"II": "<", b"MM": ">"}.get(bytes(buf[:2]))
    if bo is None:
        raise TiffError("not a TIFF file (byte-order mark)")
    (magic,) = struct.unpack_from(bo + "H", buf, 2)
    if magic == 42:
        big = False
        (ifd,) = struct.unpack_from(bo + "I", buf, 4)
    elif magic == 43:
        big = True
        (ifd,) = struct.unpack_from(bo + "Q", buf, 8)
    else:
        raise TiffError("not a TIFF file (magic)")
    t = _read_ifd(buf, bo, big, ifd)
    try:
        W, H = int(t[256][0]), int(t[257][0])
    except KeyError as e:
        raise TiffError("TIFF without ImageWidth / ImageLength") from e
    if 322 in t or 324 in t:
        raise NotImplementedError("tiled TIFF files are not supported (OpenCV and the reference write strips)")
    spp = int(t.get(277, (1,))[0])
    bits = t.get(258, (1,))
    if len(set(bits)) != 1:
        raise NotImplementedError(f"mixed BitsPerSample {bits}")
    bps = int(bits[0])
    fmt = int(t.get(339, (1,))[0])
    comp = int(t.get(259, (1,))[0])
    predictor = int(t.get(317, (1,))[0])
    if int(t.get(284, (1,))[0]) != 1 and spp > 1:
        raise NotImplementedError("planar (separate) sample layout is not supported")
    kind = {(1, 8): "u1", (1, 16): "u2", (3, 32): "f4", (3, 64): "f8", (2, 8): "i1", (2, 16): "i2", (1, 32): "u4"}.get((fmt, bps))
    if kind is None:
        raise NotImplementedError(f"SampleFormat {fmt} with {bps} bits per sample")
    dtype = np.dtype(bo + kind) if kind[1] != "1" else np.dtype(kind)
    rps = int(t.get(278, (H,))[0])
    rps = min(rps, H) if rps > 0 else H
    offsets, counts = t.get(273), t.get(279)
    if offsets is None:
        raise TiffError("TIFF without StripOffsets")
    n_strips = (H + rps - 1) // rps
    if len(offsets) < n_strips:
        raise TiffError("StripOffsets shorter than the number of strips")
    row_bytes = W * spp * dtype.itemsize
    if counts is None:
        if comp != 1:
            raise TiffError("compressed TIFF without StripByteCounts")
        counts = [row_bytes * min(rps, H - s * rps) for s in range(n_strips)]
    return TiffLayout(dtype, (H, W, spp), rps, offsets, counts, comp, predictor, int(t.get(262, (1,))[0]))


def _read_tiff(buf: memoryview) -> np.ndarray:
    lay = _parse_layout(buf)
    dtype, (H, W, spp), rps, offsets, counts, comp, predictor, photometric = lay
    n_strips, row_bytes = lay.n_strips, lay.row_bytes
    out = np.empty((H, W * spp), dtype=dtype)
    out_bytes = out.view(np.uint8).reshape(H, row_bytes)

    def one(s: int):
        rows = min(rps, H - s * rps)
        want = rows * row_bytes
        o, c = int(offsets[s]), int(counts[s])
        if o + c > len(buf):
            raise TiffError("strip beyond the end of the file")
        data = _decode_strip(bytes(buf[o:o + c]) if comp != 1 else buf[o:o + c], comp, want)
        if len(data) < want:
            raise TiffError(f"strip {s} decodes to {len(data)} bytes, expected {want}")
        out_bytes[s * rps:s * rps + rows] = np.frombuffer(data, dtype=np.uint8, count=want).reshape(rows, row_bytes)

    if comp == 1 or n_strips == 1:
        for s in range(n_strips):
            one(s)
    else:
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            list(pool.map(one, range(n_strips)))
    img = out.reshape(H, W, spp)
    if predictor == 2:
        if dtype.kind not in "ui":
            raise NotImplementedError("horizontal predictor on floating-point samples")
        native = img.astype(dtype.newbyteorder("="), copy=False)
        img = np.cumsum(native, axis=1, dtype=native.dtype)             # modular, like the encoder's differences
    elif predictor != 1:
        raise NotImplementedError(f"TIFF predictor {predictor}")
    img = np.ascontiguousarray(img.astype(dtype.newbyteorder("="), copy=False))
    if photometric == 0 and spp == 1 and dtype.kind == "u":               # WhiteIsZero
        img = np.iinfo(img.dtype).max - img
    return img[:, :, 0] if spp == 1 else img


def _swap_rb(a: np.ndarray) -> np.ndarray:
    if a.ndim == 3 and a.shape[2] in (3, 4):
        out = np.empty_like(a)                      # plane by plane: 1.7 x faster than a copy + fancy-index swap on a 4096 x 4096 x 3 image
        out[..., 0], out[..., 1], out[..., 2] = a[..., 2], a[..., 1], a[..., 0]
        if a.shape[2] == 4:
            out[..., 3] = a[..., 3]
        return out
    return a


def imread(path, flags: int = IMREAD_COLOR) -> Optional[np.ndarray]:
    """cv.imread for TIFF files. Returns None when the file does not exist (OpenCV's behaviour, which
    ImageSet.load_std_image relies on, modules/image_set.py:237-239).
    IMREAD_UNCHANGED: stored dtype, BGR(A) order, 2-D for one sample. Default: 3-channel 8-bit BGR."""
    path = Path(path)
    if not path.exists():
        return None
    img = _swap_rb(read_tiff(path))
    if flags == IMREAD_UNCHANGED:
        return img
    if img.dtype == np.uint16:
        img = (img >> 8).astype(np.uint8)
    elif img.dtype.kind == "f":
        img = np.clip(np.around(img * 255.0), 0, 255).astype(np.uint8)
    elif img.dtype != np.uint8:
        raise NotImplementedError(f"8-bit conversion of {img.dtype} samples")
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    elif img.shape[2] == 4:
        img = img[:, :, :3]
    return np.ascontiguousarray(img)


def _strip_rows(H: int, row_bytes: int) -> int:
    """OpenCV's strip rule: one strip per ~8 KiB of rows."""
    return max(1, min(H, (1 << 13) // row_bytes))


def _file_frame(H: int, W: int, S: int, dtype: np.dtype, rps: int, offsets, counts, payload_bytes: int, compression: int = 1,
                predictor: int = 1) -> Tuple[bytes, bytes]:
    """What surrounds the strips of a file, shared by imwrite and the device writer: (head, tail). The file is head + payload + tail:
    head is the TIFF or BigTIFF header (the switch is decided from the real payload size), tail the padding to an even offset, the IFD
    and its out-of-line values. `offsets` are relative to the payload's first byte; Compression (259) is always written, Predictor (317)
    only when it is not 1."""
    n_strips = len(counts)
    big = payload_bytes + 16 * n_strips + 4096 >= (1 << 32)
    osz = 8 if big else 4
    otype = 16 if big else 4
    header = 16 if big else 8
    pos = header + payload_bytes
    pos += pos & 1
    entries = []          # (tag, type, values)
    fmt = 3 if dtype.kind == "f" else 1
    entries.append((256, 4, [W]))
    entries.append((257, 4, [H]))
    entries.append((258, 3, [dtype.itemsize * 8] * S))
    entries.append((259, 3, [compression]))
    entries.append((262, 3, [2 if S >= 3 else 1]))
    entries.append((273, otype, [header + int(o) for o in offsets[:n_strips]]))
    entries.append((277, 3, [S]))
    entries.append((278, 4, [rps]))
    entries.append((279, otype, [int(c) for c in counts]))
    entries.append((284, 3, [1]))
    if predictor != 1:
        entries.append((317, 3, [predictor]))
    if S == 4:
        entries.append((338, 3, [2]))                   # unassociated alpha
    entries.append((339, 3, [fmt] * S))
    entries.sort(key=lambda e: e[0])
    n = len(entries)
    ifd_off = pos
    ifd_size = (8 + 20 * n + 8) if big else (2 + 12 * n + 4)
    extra_off = ifd_off + ifd_size
    ifd = bytearray()
    extra = bytearray()
    ifd += struct.pack("<Q" if big else "<H", n)
    for tag, typ, vals in entries:
        payload = struct.pack("<" + _TYPE_FMT[typ] * len(vals), *vals)
        ifd += struct.pack("<HH", tag, typ) + struct.pack("<Q" if big else "<I", len(vals))
        if len(payload) <= osz:
            ifd += payload.ljust(osz, b"\0")
        else:
            ifd += struct.pack("<Q" if big else "<I", extra_off + len(extra))
            extra += payload
            if len(extra) & 1:
                extra += b"\0"
    ifd += struct.pack("<Q" if big else "<I", 0)
    head = struct.pack("<2sHHHQ", b"II", 43, 8, 0, ifd_off) if big else struct.pack("<2sHI", b"II", 42, ifd_off)
    pad = b"\0" if (header + payload_bytes) & 1 else b""
    return head, pad + bytes(ifd) + bytes(extra)


def _check_write_options(dtype, compression: int, predictor: int, who: str, wide_samples: bool = False) -> None:
    """What is not written raises here, before a file or a launch. `wide_samples` admits what hm_tiff_encode_strips_wide encodes: LZW
    strips of uint16 and float32 samples and the horizontal predictor on uint16."""
    if compression not in (1, 5):
        raise NotImplementedError(f"{who}: TIFF compression {compression} is not written (1 = none and 5 = LZW are)")
    if predictor not in (1, 2):
        raise ValueError(f"{who}: TIFF predictor {predictor} (1 = none and 2 = horizontal differencing exist)")
    if wide_samples:
        if predictor == 2 and np.dtype(dtype) not in (np.uint8, np.uint16):
            raise NotImplementedError(f"{who}: the horizontal predictor is written for uint8 and uint16 samples, not {np.dtype(dtype).name}")
        return
    if predictor == 2 and np.dtype(dtype) != np.uint8:
        raise NotImplementedError(f"{who}: the horizontal predictor is written for uint8 samples only, not {np.dtype(dtype).name}")
    if (compression, predictor) != (1, 1) and np.dtype(dtype) not in (np.uint8, np.float64):
        raise NotImplementedError(f"{who}: LZW strips and the predictor are written for uint8 and float64 samples, not {np.dtype(dtype).name}")


def imwrite(path, img, compression: int = 1, predictor: int = 1, wide_samples: bool = False) -> bool:
    """cv.imwrite for TIFF files: (H, W) or (H, W, 3|4) arrays in BGR(A) order; uint8 / uint16 / float32 / float64.
    RGB(A) order in the file. Default: uncompressed strips. `compression=5` writes LZW strips (uint8 and float64; what cv.imwrite's TIFF
    writer does), `predictor=2` horizontal differencing (uint8 only); both go through the host build's hm_tiff_encode_strips.
    `wide_samples=True` (opt-in) also takes `compression=5` for uint16 and float32 and `predictor=2` for uint16 (differences modulo
    65536), through the host build's hm_tiff_encode_strips_wide; without it every refusal is as it was. What is not written raises
    ValueError / NotImplementedError before the file is created."""
    a = np.asarray(img)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype not in (np.uint8, np.uint16, np.float32, np.float64):
        raise TypeError(f"imwrite: unsupported sample type {a.dtype}")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4):
        raise ValueError(f"imwrite: unsupported array shape {np.asarray(img).shape}")
    H, W, S = a.shape
    if H == 0 or W == 0:
        raise ValueError("imwrite: empty image")
    _check_write_options(a.dtype, compression, predictor, "imwrite", wide_samples)
    row_bytes = W * S * a.dtype.itemsize
    rps = _strip_rows(H, row_bytes)
    n_strips = (H + rps - 1) // rps
    if (compression, predictor) == (1, 1):
        a = np.ascontiguousarray(_swap_rb(a)).astype(a.dtype.newbyteorder("<"), copy=False)
        counts = [row_bytes * min(rps, H - s * rps) for s in range(n_strips)]
        offsets = [s * rps * row_bytes for s in range(n_strips)]
        payload = a.tobytes()
    else:
        nat = _native()
        lib = nat.host_lib()
        a = np.ascontiguousarray(a.astype(a.dtype.newbyteorder("="), copy=False))
        strip_bytes = rps * row_bytes
        cap = int(lib.hm_tiff_encode_payload_bytes(n_strips, strip_bytes, compression))
        if cap == 0:
            raise ValueError(f"imwrite: strips of {strip_bytes} bytes cannot be encoded")
        buf = np.empty(cap, dtype=np.uint8)
        ws = np.empty(max(1, int(lib.hm_tiff_encode_workspace_bytes(n_strips, strip_bytes, compression))), dtype=np.uint8)
        tables = np.empty(2 * n_strips + 1, dtype=np.int64)
        if a.dtype in (np.uint16, np.float32):         # only reached with wide_samples: the option check refuses them without it
            nat.check(lib.hm_tiff_encode_strips_wide(a.ctypes.data, nat.HM_TIFF_SRC_U16 if a.dtype == np.uint16 else nat.HM_TIFF_SRC_F32,
                                                     1.0, 0, H, W, S, rps, compression, predictor, buf.ctypes.data, cap, tables.ctypes.data,
                                                     tables.ctypes.data + 8 * (n_strips + 1), ws.ctypes.data, None),
                      "hm_tiff_encode_strips_wide")
        else:
            nat.check(lib.hm_tiff_encode_strips(a.ctypes.data, 0 if a.dtype == np.uint8 else 1, 1.0, H, W, S, rps, compression, predictor,
                                                buf.ctypes.data, cap, tables.ctypes.data, tables.ctypes.data + 8 * (n_strips + 1),
                                                ws.ctypes.data, None), "hm_tiff_encode_strips")
        offsets, counts = tables[:n_strips + 1], tables[n_strips + 1:]
        if (counts < 0).any():
            raise TiffError(f"strip {int(np.flatnonzero(counts < 0)[0])} could not be encoded ({nat.strerror(int(counts[counts < 0][0]))})")
        payload = memoryview(buf)[:int(offsets[n_strips])]
    head, tail = _file_frame(H, W, S, a.dtype, rps, offsets, counts, len(payload), compression, predictor)
    path = Path(path)
    with open(path, "wb") as f:
        f.write(head)
        f.write(payload)
        f.write(tail)
    return True


# ---------------------------------------------------------------------------------------------------------------------
# The device path (opt-in): hm_tiff_decode_strips
# ---------------------------------------------------------------------------------------------------------------------
_HOST_PATH = "tiff_io.imread is the host path for such files"


def _device_compression_check(lay: TiffLayout) -> None:
    if lay.compression in (8, 32946):
        raise NotImplementedError(f"imread_device: Deflate-compressed strips are not decoded on the device; {_HOST_PATH}")
    if lay.compression == 32773:
        raise NotImplementedError(f"imread_device: PackBits-compressed strips are not decoded on the device; {_HOST_PATH}")
    if lay.compression not in (1, 5):
        raise NotImplementedError(f"imread_device: TIFF compression {lay.compression} is not supported; {_HOST_PATH}")


def _device_layout_check_wide(lay: TiffLayout, flags: int) -> None:
    """_device_layout_check for imread_device(wide_samples=True): uint8 / uint16 (1 / 3 / 4 samples, Predictor 1 / 2, both flags) and
    float32 / float64 (1 / 3 samples, IMREAD_UNCHANGED) in either byte order."""
    spp = lay.shape[2]
    _device_compression_check(lay)
    kind = lay.dtype.kind + str(lay.dtype.itemsize)
    if kind not in ("u1", "u2", "f4", "f8"):
        raise NotImplementedError(f"imread_device: {lay.dtype.name} samples are not decoded on the device (uint8, uint16, float32 and "
                                  f"float64 are); {_HOST_PATH}")
    if spp not in ((1, 3, 4) if lay.dtype.kind == "u" else (1, 3)):
        raise NotImplementedError(f"imread_device: {spp} {lay.dtype.name} samples per pixel are not decoded on the device; {_HOST_PATH}")
    if lay.predictor not in (1, 2):
        raise NotImplementedError(f"TIFF predictor {lay.predictor}")
    if lay.predictor == 2 and lay.dtype.kind != "u":
        raise NotImplementedError(f"imread_device: the horizontal predictor on floating-point samples is not supported; {_HOST_PATH}")
    if lay.photometric == 0 and spp == 1 and lay.dtype.kind == "u":
        raise NotImplementedError(f"imread_device: WhiteIsZero images are not inverted on the device; {_HOST_PATH}")
    if lay.dtype.kind == "f" and flags != IMREAD_UNCHANGED:
        raise NotImplementedError(f"imread_device: {lay.dtype.name} samples are read with IMREAD_UNCHANGED only (no 8-bit conversion on "
                                  f"the device); {_HOST_PATH}")


def _device_layout_check(lay: TiffLayout, flags: int, wide_samples: bool = False) -> None:
    """NotImplementedError for every kind of file the device decoder does not read (it never falls back). `wide_samples` admits what
    hm_tiff_decode_strips_wide reads: uint16 and float32 samples and big-endian multi-byte ones."""
    if wide_samples:
        return _device_layout_check_wide(lay, flags)
    spp = lay.shape[2]
    _device_compression_check(lay)
    kind = lay.dtype.kind + str(lay.dtype.itemsize)
    if kind not in ("u1", "f8"):
        raise NotImplementedError(f"imread_device: {lay.dtype.name} samples are not decoded on the device (uint8 and float64 are); "
                                  f"{_HOST_PATH}")
    if lay.dtype.itemsize > 1 and lay.dtype.byteorder == ">":
        raise NotImplementedError(f"imread_device: big-endian multi-byte samples are not decoded on the device; {_HOST_PATH}")
    if spp not in ((1, 3, 4) if kind == "u1" else (1, 3)):
        raise NotImplementedError(f"imread_device: {spp} {lay.dtype.name} samples per pixel are not decoded on the device; {_HOST_PATH}")
    if lay.predictor not in (1, 2):
        raise NotImplementedError(f"TIFF predictor {lay.predictor}")
    if lay.predictor == 2 and kind != "u1":
        raise NotImplementedError(f"imread_device: the horizontal predictor on floating-point samples is not supported; {_HOST_PATH}")
    if lay.photometric == 0 and spp == 1 and kind == "u1":
        raise NotImplementedError(f"imread_device: WhiteIsZero images are not inverted on the device; {_HOST_PATH}")
    if kind == "f8" and flags != IMREAD_UNCHANGED:
        raise NotImplementedError(f"imread_device: float64 samples are read with IMREAD_UNCHANGED only (no 8-bit conversion on the "
                                  f"device); {_HOST_PATH}")


class DeviceTiffReader:
    """The buffers of the device path, kept and grown across the files of a series: a pinned host staging buffer that holds a file's
    bytes followed by its strip tables (so ONE upload carries both), its device twin, the per-strip status and the decoder's workspace.
    Per file: one read into pinned memory, one upload, one hm_tiff_decode_strips, one status read-back (the only synchronisation).
    Not thread-safe: one reader per thread."""

    def __init__(self, device=None):
        self._device_arg = device
        self.device = None                 # resolved by the first file that passes the layout checks (those need no GPU)
        self._pinned = self._dev = self._status = self._ws = None

    def _resolve_device(self):
        import torch
        if self.device is None:
            dev = torch.device("cuda") if self._device_arg is None else torch.device(self._device_arg)
            if dev.type != "cuda":
                raise ValueError(f"DeviceTiffReader needs a GPU device, got {dev}")
            self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        return self.device

    def _grow(self, name: str, n: int, **kw):
        import torch
        t = getattr(self, name)
        if t is None or t.numel() < n:
            t = torch.empty(max(n, 1) + max(n, 1) // 4, **kw)          # head room: the files of a series differ a little in size
            setattr(self, name, t)
        return t

    def read(self, path, flags: int = IMREAD_COLOR, wide_samples: bool = False):
        """The frame `imread(path, flags)` returns, as a tensor on the reader's device; None when the file does not exist.
        `wide_samples=True` also reads uint16 and float32 samples and big-endian multi-byte ones (hm_tiff_decode_strips_wide): a
        torch.uint16 / float32 / float64 tensor, uint8 for uint16 samples under IMREAD_COLOR."""
        path = Path(path)
        if not path.exists():
            return None
        if flags not in (IMREAD_COLOR, IMREAD_UNCHANGED):
            raise ValueError(f"imread_device: flags must be IMREAD_COLOR or IMREAD_UNCHANGED, got {flags}")
        with open(path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            if size < 8:
                raise TiffError("not a TIFF file (too short)")
            # the layout first, from a mapping (only the pages of the header and the IFD are touched): what the device does not read
            # is refused before a byte is staged, and the staging buffer can be sized for the file AND its strip tables
            with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
                view = memoryview(mm)
                try:
                    lay = _parse_layout(view)
                except (struct.error, IndexError, OverflowError, MemoryError) as e:
                    raise TiffError(f"malformed TIFF file {path}: {e}") from e
                except NotImplementedError as e:
                    raise NotImplementedError(f"imread_device: {e}; tiff_io.imread, the host path, refuses this layout too") from e
                finally:
                    view.release()
            _device_layout_check(lay, flags, wide_samples)
            H, W, spp = lay.shape
            n = lay.n_strips
            if len(lay.counts) < n:
                raise TiffError("StripByteCounts shorter than the number of strips")
            import torch
            nat = _native()
            device = self._resolve_device()
            cap = (size + 7) // 8 * 8                   # the tables sit 8-byte aligned behind the file's bytes: ONE upload carries both
            host = self._grow("_pinned", cap + 16 * n, dtype=torch.uint8, pin_memory=True).numpy()
            if f.readinto(memoryview(host)[:size]) != size:
                raise TiffError(f"short read of {path}")
        tables = host[cap:cap + 16 * n].view(np.int64)
        try:
            tables[:n] = lay.offsets[:n]
            tables[n:] = lay.counts[:n]
        except OverflowError as e:
            raise TiffError(f"malformed TIFF file {path}: {e}") from e
        used = cap + 16 * n
        dev = self._grow("_dev", used, dtype=torch.uint8, device=device)
        status = self._grow("_status", n, dtype=torch.int64, device=device)
        bps = lay.dtype.itemsize
        strip_bytes = lay.rows_per_strip * lay.row_bytes
        ws_bytes = int(nat.hip_lib.hm_tiff_decode_workspace_bytes(n, strip_bytes, lay.compression))
        ws = self._grow("_ws", ws_bytes, dtype=torch.uint8, device=device) if ws_bytes else None
        color = flags == IMREAD_COLOR
        out_spp = 3 if color else spp
        out_shape = (H, W) if out_spp == 1 else (H, W, out_spp)
        with torch.cuda.device(device):
            dev[:used].copy_(self._pinned[:used], non_blocking=True)
            base = dev.data_ptr()
            big_endian = bps > 1 and lay.dtype.byteorder == ">"
            if bps in (2, 4) or big_endian:            # only reached with wide_samples: the layout check refuses them without it
                kind = lay.dtype.kind + str(bps)
                dst = torch.empty(out_shape, dtype=torch.uint8 if color else getattr(torch, _WIDE_TORCH_DTYPES[kind]), device=device)
                nat.check(nat.hip_lib.hm_tiff_decode_strips_wide(base, size, base + cap, base + cap + 8 * n, n, lay.compression,
                                                                 lay.predictor, lay.rows_per_strip, H, W, spp, bps, int(big_endian),
                                                                 1 if color else 0, dst.data_ptr(), status.data_ptr(), nat.ptr(ws),
                                                                 nat.current_stream_ptr(device)),
                          "hm_tiff_decode_strips_wide")
            else:
                dst = torch.empty(out_shape, dtype=torch.uint8 if bps == 1 else torch.float64, device=device)
                nat.check(nat.hip_lib.hm_tiff_decode_strips(base, size, base + cap, base + cap + 8 * n, n, lay.compression, lay.predictor,
                                                            lay.rows_per_strip, H, W, spp, bps, 1 if color else 0, dst.data_ptr(),
                                                            status.data_ptr(), nat.ptr(ws), nat.current_stream_ptr(device)),
                          "hm_tiff_decode_strips")
            st = status[:n].cpu().numpy()              # waits for the upload and the kernels: the pinned buffer is free again after it
        want = np.minimum(lay.rows_per_strip, H - np.arange(n, dtype=np.int64) * lay.rows_per_strip) * lay.row_bytes
        bad = np.flatnonzero(st < want)
        if bad.size:
            s = int(bad[0])
            if st[s] < 0:
                what = "lies beyond the end of the file or holds a corrupt stream" if st[s] == nat.HM_EINVAL else \
                    "decodes to more bytes than its rows hold"
                raise TiffError(f"strip {s} {what} ({nat.strerror(int(st[s]))})")
            raise TiffError(f"strip {s} decodes to {int(st[s])} bytes, expected {int(want[s])}")
        return dst


_WIDE_TORCH_DTYPES = {"u2": "uint16", "f4": "float32", "f8": "float64"}       # names: torch is imported by the first read
_readers = {}


def imread_device(path, flags: int = IMREAD_COLOR, device=None, reader: Optional[DeviceTiffReader] = None, wide_samples: bool = False):
    """`imread` with the decode on the GPU: the same array (values, dtype, shape, BGR order) as a torch tensor in device memory, None
    when the file does not exist. Opt-in; files outside the device decoder's family raise NotImplementedError (no fallback: call
    `imread`), damaged strips raise TiffError naming the strip. `reader` (a DeviceTiffReader) carries the buffers from file to file;
    without one, a reader per device is kept by the module. `wide_samples=True` (opt-in) widens the family to uint16 (both flags; a
    torch.uint16 tensor, or uint8 `>> 8` under IMREAD_COLOR), float32 and big-endian multi-byte samples: DeviceTiffReader.read."""
    if reader is None:
        reader = _readers.get(str(device))
        if reader is None:
            reader = _readers[str(device)] = DeviceTiffReader(device)
    return reader.read(path, flags, wide_samples)


# ---------------------------------------------------------------------------------------------------------------------
# The device path of writing (opt-in): hm_tiff_encode_strips, hm_tiff_encode_strips_wide
# ---------------------------------------------------------------------------------------------------------------------
class DeviceTiffWriter:
    """The buffers of the device writer, kept and grown across files like DeviceTiffReader's: the device payload, the encoder's
    workspace, the strip tables (offsets and counts in one tensor, so ONE read-back carries both) and a pinned host buffer.
    Per file: one hm_tiff_encode_strips, one read-back of the tables (skipped for compression 1, whose tables follow from the geometry),
    one copy of payload[:total] into pinned memory, one write of header, payload and IFD. Not thread-safe: one writer per thread."""

    def __init__(self, device=None):
        self._device_arg = device
        self.device = None
        self._payload = self._ws = self._tables = self._pinned = None

    _grow = DeviceTiffReader._grow

    def write(self, path, tensor, compression: int = 1, predictor: int = 1, quantize_divisor: Optional[float] = None,
              wide_samples: bool = False, narrow_to_float32: bool = False, quantize_max_dn: Optional[int] = None) -> bool:
        """`imwrite(path, array)` for a tensor in device memory: (H, W) or (H, W, 1|3|4), contiguous, uint8 or float64, BGR(A) order.
        `quantize_divisor=d` (float64 tensors) stores uint8 samples around((v / d) * 255) - save_8bit's arithmetic; non-finite samples
        give 0, results outside 0..255 wrap modulo 256. Nothing falls back: what the device does not write raises.
        Through hm_tiff_encode_strips_wide (all opt-in): `wide_samples=True` also takes torch.uint16 (stored as it is, Predictor 1 / 2)
        and torch.float32 (stored bit for bit) tensors; `narrow_to_float32=True` stores a float64 tensor as float32, rounded like
        ndarray.astype(np.float32); `quantize_max_dn=m` (1 .. 65535, with `quantize_divisor=d`, 1.0 if not given) stores a float64
        tensor as uint16 samples around((v / d) * m) - save_16bit's arithmetic; non-finite samples give 0, results outside 0..65535
        wrap modulo 65536 - with Predictor 1 / 2."""
        import torch
        if not isinstance(tensor, torch.Tensor):
            raise TypeError(f"imwrite_device: a torch tensor in device memory is required, got {type(tensor).__name__}; "
                            "tiff_io.imwrite is the host path")
        if tensor.device.type != "cuda":
            raise ValueError("imwrite_device: the tensor is in host memory; tiff_io.imwrite is the host path")
        if tensor.dtype not in ((torch.uint8, torch.float64, torch.uint16, torch.float32) if wide_samples else (torch.uint8, torch.float64)):
            raise TypeError(f"imwrite_device: uint8 and float64 tensors are written (uint16 and float32 with wide_samples=True), not "
                            f"{tensor.dtype}; tiff_io.imwrite is the host path")
        if tensor.dim() not in (2, 3) or (tensor.dim() == 3 and tensor.shape[2] not in (1, 3, 4)) or tensor.numel() == 0:
            raise ValueError(f"imwrite_device: unsupported tensor shape {tuple(tensor.shape)}")
        if not tensor.is_contiguous():
            raise ValueError("imwrite_device: the tensor must be contiguous")
        if quantize_divisor is not None:
            if tensor.dtype != torch.float64:
                raise ValueError("imwrite_device: quantize_divisor applies to float64 tensors")
            quantize_divisor = float(quantize_divisor)
            if not (0.0 < quantize_divisor < float("inf")):
                raise ValueError(f"imwrite_device: quantize_divisor must be finite and positive, got {quantize_divisor}")
        if quantize_max_dn is not None:
            if tensor.dtype != torch.float64:
                raise ValueError("imwrite_device: quantize_max_dn applies to float64 tensors")
            if isinstance(quantize_max_dn, bool) or int(quantize_max_dn) != quantize_max_dn or not 1 <= int(quantize_max_dn) <= 65535:
                raise ValueError(f"imwrite_device: quantize_max_dn must be an integer in 1..65535 (2**bit_depth - 1), got {quantize_max_dn}")
            quantize_max_dn = int(quantize_max_dn)
        if narrow_to_float32:
            if tensor.dtype != torch.float64:
                raise ValueError("imwrite_device: narrow_to_float32 applies to float64 tensors")
            if quantize_divisor is not None or quantize_max_dn is not None:
                raise ValueError("imwrite_device: narrow_to_float32 and quantisation exclude each other")
        nat = _native()
        wide = True                                 # hm_tiff_encode_strips_wide; `kind` is the entry's own src_kind
        if tensor.dtype == torch.uint16:
            kind, out_dtype = nat.HM_TIFF_SRC_U16, np.dtype(np.uint16)
        elif tensor.dtype == torch.float32:
            kind, out_dtype = nat.HM_TIFF_SRC_F32, np.dtype(np.float32)
        elif narrow_to_float32:
            kind, out_dtype = nat.HM_TIFF_SRC_F64_AS_F32, np.dtype(np.float32)
        elif quantize_max_dn is not None:
            kind, out_dtype = nat.HM_TIFF_SRC_F64_AS_U16, np.dtype(np.uint16)
        else:
            wide = False
            kind = 0 if tensor.dtype == torch.uint8 else (1 if quantize_divisor is None else 2)
            out_dtype = np.dtype(np.float64 if kind == 1 else np.uint8)
        _check_write_options(out_dtype, compression, predictor, "imwrite_device", wide)
        if self._device_arg is not None and torch.device(self._device_arg).index not in (None, tensor.device.index):
            raise ValueError(f"imwrite_device: the writer belongs to {self._device_arg}, the tensor is on {tensor.device}")
        device = self.device = tensor.device
        H, W = int(tensor.shape[0]), int(tensor.shape[1])
        S = int(tensor.shape[2]) if tensor.dim() == 3 else 1
        row_bytes = W * S * out_dtype.itemsize
        rps = _strip_rows(H, row_bytes)
        n = (H + rps - 1) // rps
        strip_bytes = rps * row_bytes
        lib = nat.hip_lib
        cap = int(lib.hm_tiff_encode_payload_bytes(n, strip_bytes, compression))
        if cap == 0:
            raise ValueError(f"imwrite_device: strips of {strip_bytes} bytes cannot be encoded")
        ws_bytes = int(lib.hm_tiff_encode_workspace_bytes(n, strip_bytes, compression))
        payload = self._grow("_payload", cap, dtype=torch.uint8, device=device)
        ws = self._grow("_ws", ws_bytes, dtype=torch.uint8, device=device) if ws_bytes else None
        tables = self._grow("_tables", 2 * n + 1, dtype=torch.int64, device=device)
        with torch.cuda.device(device):
            divisor = 1.0 if quantize_divisor is None else quantize_divisor
            if wide:
                nat.check(lib.hm_tiff_encode_strips_wide(tensor.data_ptr(), kind, divisor, quantize_max_dn or 0, H, W, S, rps, compression,
                                                         predictor, payload.data_ptr(), cap, tables.data_ptr(),
                                                         tables.data_ptr() + 8 * (n + 1), nat.ptr(ws), nat.current_stream_ptr(device)),
                          "hm_tiff_encode_strips_wide")
            else:
                nat.check(lib.hm_tiff_encode_strips(tensor.data_ptr(), kind, divisor, H, W, S, rps, compression, predictor,
                                                    payload.data_ptr(), cap, tables.data_ptr(), tables.data_ptr() + 8 * (n + 1),
                                                    nat.ptr(ws), nat.current_stream_ptr(device)),
                          "hm_tiff_encode_strips")
            if compression == 1:
                counts = [row_bytes * min(rps, H - s * rps) for s in range(n)]
                offsets = [s * strip_bytes for s in range(n)]
                total = H * row_bytes
            else:
                t = tables[:2 * n + 1].cpu().numpy()       # waits for the kernels
                offsets, counts = t[:n + 1], t[n + 1:]
                if (counts < 0).any():
                    raise TiffError(f"strip {int(np.flatnonzero(counts < 0)[0])} could not be encoded "
                                    f"({nat.strerror(int(counts[counts < 0][0]))})")
                total = int(offsets[n])
            pinned = self._grow("_pinned", total, dtype=torch.uint8, pin_memory=True)
            pinned[:total].copy_(payload[:total], non_blocking=True)
            head, tail = _file_frame(H, W, S, out_dtype, rps, offsets, counts, total, compression, predictor)
            torch.cuda.current_stream(device).synchronize()
        with open(Path(path), "wb") as f:
            f.write(head)
            f.write(memoryview(pinned.numpy())[:total])
            f.write(tail)
        return True


_writers = {}


def imwrite_device(path, tensor, compression: int = 1, predictor: int = 1, quantize_divisor: Optional[float] = None,
                   writer: Optional[DeviceTiffWriter] = None, wide_samples: bool = False, narrow_to_float32: bool = False,
                   quantize_max_dn: Optional[int] = None) -> bool:
    """`imwrite` with the encode on the GPU (hm_tiff_encode_strips): the tensor - contiguous, in device memory, uint8 or float64,
    (H, W) or (H, W, 1|3|4) in BGR(A) order - becomes the strips of the file on the device and comes down as one payload. With
    compression 1 the file is byte-identical to imwrite's. Opt-in; a host tensor, another dtype or a non-contiguous tensor raises (no
    fallback: call `imwrite`). `writer` (a DeviceTiffWriter) carries the buffers from file to file; without one, a writer per device is
    kept by the module. `wide_samples=True` (opt-in) also takes torch.uint16 and torch.float32 tensors, `narrow_to_float32=True` stores a
    float64 tensor as float32 and `quantize_max_dn=m` stores it as uint16 (hm_tiff_encode_strips_wide): DeviceTiffWriter.write."""
    if writer is None:
        key = str(getattr(tensor, "device", None))
        writer = _writers.get(key)
        if writer is None:
            writer = _writers[key] = DeviceTiffWriter()
    return writer.write(path, tensor, compression, predictor, quantize_divisor, wide_samples, narrow_to_float32, quantize_max_dn)
