"""The wide TIFF writing path (hm_tiff_encode_strips_wide, tiff_io.imwrite(wide_samples=True), ImageSet.save_16bit / save_32bit) as far
as a box without a GPU can check it, and the helpers its GPU tests share (tests/test_gpu_tiff_encode_wide.py).

The host build's hm_tiff_encode_strips_wide runs the row text both builds share (csrc/hm_tiff_wide_enc_body.h), so every strip is
pinned here, byte for byte, against an expectation NumPy builds - the R/B swap, the quantisation or narrowing, the differences modulo
65536 and the little-endian bytes - encoded by lzw_encode of tests/test_tiff_device_host.py; the GPU tests then compare the device
call with the host build's. Also here: Predictor 2 where differences wrap, the uint16 quantisation with exact ties, the float32
narrowing on subnormals, ties and overflow, files read back by imread and Pillow, the argument rules in their order, ImageSet on the
host backend, and the stand-alone sanitizer program of the row text."""
import itertools
import pathlib
import subprocess

import numpy as np
import pytest

from camera_linearity_amd import tiff_io as T
from test_tiff_device_host import bgr, lzw_encode

ROOT = pathlib.Path(__file__).resolve().parent.parent
U16, F32, F64_AS_F32, F64_AS_U16 = range(4)          # HM_TIFF_SRC_* of include/hdrmerge.h
SRC_DTYPE = {U16: np.uint16, F32: np.float32, F64_AS_F32: np.float64, F64_AS_U16: np.float64}
OUT_BYTES = {U16: 2, F32: 4, F64_AS_F32: 4, F64_AS_U16: 2}
WRAP = np.array([0, 65535, 1, 32768, 32767], dtype=np.uint16)     # neighbours whose differences wrap both ways


# ---------------------------------------------------------------------------------------------------------------------
# helpers (shared with tests/test_gpu_tiff_encode_wide.py)
# ---------------------------------------------------------------------------------------------------------------------
def quantise_u16_reference(img, divisor, max_dn):
    """around((v / divisor) * max_dn) reduced modulo 65536, non-finite samples and |r| >= 2^63 -> 0: the statement of kind 3."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.around((np.asarray(img, dtype=np.float64) / divisor) * max_dn)
        ok = np.isfinite(r) & (np.abs(r) < 2.0 ** 63)
        r = np.where(ok, r, 0.0)
        return np.mod(r, 65536.0).astype(np.uint16)               # exact: |r| < 2^63 doubles are integers, fmod is exact


def stored_reference(img, kind, divisor=1.0, max_dn=0):
    """The stored samples of a BGR(A) array, still in memory order."""
    a = np.asarray(img)
    if kind == F64_AS_U16:
        return quantise_u16_reference(a, divisor, max_dn)
    if kind == F64_AS_F32:
        with np.errstate(over="ignore"):
            return a.astype(np.float32)
    return a


def packed_reference(img, kind, divisor, max_dn, predictor):
    """What the pack step must produce: stored samples in file order, Predictor 2 applied per row modulo 65536, little-endian."""
    st = stored_reference(img, kind, divisor, max_dn)
    st = st[:, :, None] if st.ndim == 2 else st
    f = bgr(st) if st.shape[2] >= 3 else st
    if predictor == 2:
        assert f.dtype == np.uint16
        f = np.concatenate([f[:, :1], np.diff(f, axis=1)], axis=1)          # uint16 arithmetic: modulo 65536
    return np.ascontiguousarray(f.astype(f.dtype.newbyteorder("<"), copy=False))


def abi_encode_wide(lib, img, kind, divisor=1.0, max_dn=0, rows_per_strip=1, compression=5, predictor=1, on_device=False):
    """A BGR(A) array through hm_tiff_encode_strips_wide of `lib`: (payload[:total], offsets, counts, rc). Host arrays for the host
    build; with on_device the arrays are torch tensors on the GPU with 4 KiB of 0xA5 behind payload and workspace, which must survive."""
    a = np.ascontiguousarray(img)
    assert a.dtype == SRC_DTYPE[kind]
    a3 = a[:, :, None] if a.ndim == 2 else a
    H, W, S = a3.shape
    rps = min(rows_per_strip, H)
    n = -(-H // rps)
    strip_bytes = rps * W * S * OUT_BYTES[kind]
    cap = int(lib.hm_tiff_encode_payload_bytes(n, strip_bytes, compression))
    wsb = int(lib.hm_tiff_encode_workspace_bytes(n, strip_bytes, compression))
    assert cap > 0 and (wsb > 0) == (compression == 5)
    tail = 4096
    if on_device:
        import torch
        from camera_linearity_amd import _native as nat
        dev = torch.device("cuda")
        src = torch.from_numpy(a).to(dev)
        payload = torch.full((cap + tail,), 0xA5, dtype=torch.uint8, device=dev)
        ws = torch.full((max(wsb, 16) + tail,), 0xA5, dtype=torch.uint8, device=dev)
        tables = torch.full((2 * n + 1,), -99, dtype=torch.int64, device=dev)
        rc = lib.hm_tiff_encode_strips_wide(src.data_ptr(), kind, divisor, max_dn, H, W, S, rows_per_strip, compression, predictor,
                                            payload.data_ptr(), cap, tables.data_ptr(), tables.data_ptr() + 8 * (n + 1),
                                            ws.data_ptr() if wsb else None, nat.current_stream_ptr(dev))
        torch.cuda.synchronize()
        payload, ws, tables = payload.cpu().numpy(), ws.cpu().numpy(), tables.cpu().numpy()
        assert (payload[cap:] == 0xA5).all() and (ws[max(wsb, 16):] == 0xA5).all(), "a byte behind the stated sizes was written"
        offsets, counts = tables[:n + 1], tables[n + 1:]
    else:
        payload = np.full(cap, 0xA5, dtype=np.uint8)
        ws = np.full(max(wsb, 16), 0xA5, dtype=np.uint8)
        offsets = np.full(n + 1, -99, dtype=np.int64)
        counts = np.full(n, -99, dtype=np.int64)
        rc = lib.hm_tiff_encode_strips_wide(a.ctypes.data, kind, divisor, max_dn, H, W, S, rows_per_strip, compression, predictor,
                                            payload.ctypes.data, cap, offsets.ctypes.data, counts.ctypes.data,
                                            ws.ctypes.data if wsb else None, None)
    if rc != 0:
        return None, offsets, counts, rc
    total = int(offsets[n])
    assert 0 <= total <= cap
    return payload[:total].copy(), offsets.copy(), counts.copy(), rc


def check_against_reference(img, kind, divisor, max_dn, rows_per_strip, compression, predictor, payload, offsets, counts, lib):
    """Compression 1: the payload is the packed image and the tables follow from the geometry. Compression 5: every strip equals
    lzw_encode of the packed strip; offsets are multiples of 16, counts exact, gaps zero, last = total."""
    ref = packed_reference(img, kind, divisor, max_dn, predictor)
    H = ref.shape[0]
    rps = min(rows_per_strip, H)
    n = -(-H // rps)
    row = ref[0].nbytes
    if compression == 1:
        assert payload.tobytes() == ref.tobytes()
        assert list(offsets) == [s * rps * row for s in range(n)] + [H * row]
        assert list(counts) == [row * min(rps, H - s * rps) for s in range(n)]
        return
    pos = 0
    for s in range(n):
        raw = ref[s * rps:(s + 1) * rps].tobytes()
        want = lzw_encode(raw, eoi=True)
        assert offsets[s] == pos and pos % 16 == 0, (s, offsets[s], pos)
        assert counts[s] == len(want), (s, counts[s], len(want))
        assert len(want) <= lib.hm_tiff_encode_bound(len(raw))
        assert payload[pos:pos + len(want)].tobytes() == want, s
        end = -(-(pos + len(want)) // 16) * 16
        assert not payload[pos + len(want):end].any(), f"gap after strip {s} is not zero"
        pos = end
    assert offsets[n] == pos == len(payload)


def source_image(kind, H, W, samples, seed, divisor=1.0):
    """Half smooth, half noise, in the source type of `kind`: 12-bit DNs, float32 / float64 values in [0, divisor) with a few above
    the range (kind 3 then stores a few samples above max_dn)."""
    rng = np.random.default_rng(seed)
    ramp = (np.add.outer(np.arange(H) * 37, np.arange(W) * 29)[:, :, None] + np.arange(samples) * 400) % 4096
    noise = rng.integers(0, 4096, ramp.shape)
    dn = np.where(np.arange(W)[None, :, None] < W // 2, ramp, noise)
    if kind == U16:
        img = dn.astype(np.uint16)
        img[0, 0, 0] = 65535
    else:
        img = (dn / 4095.0 * divisor * np.where(rng.random(dn.shape) < 0.02, 1.5, 1.0)).astype(SRC_DTYPE[kind])
    return img[:, :, 0] if samples == 1 else img


WIDTHS = (1, 63, 64, 65, 129)


def strip_cases():
    """(name, array, kind, divisor, max_dn, rows_per_strip, compression, predictor): H = 9 with 4 rows per strip (a short last strip of
    one row), widths around the 64-lane step, 1 / 3 / 4 samples, the four kinds, both compressions, both predictors where they exist."""
    for W, samples, kind, compression in itertools.product(WIDTHS, (1, 3, 4), (U16, F32, F64_AS_F32, F64_AS_U16), (1, 5)):
        divisor, max_dn = (3.7, 4095) if kind == F64_AS_U16 else (1.0, 0)
        img = source_image(kind, 9, W, samples, seed=W * 10 + samples, divisor=divisor)
        for predictor in ((1, 2) if OUT_BYTES[kind] == 2 else (1,)):
            yield f"k{kind} w{W} s{samples} c{compression} p{predictor}", img, kind, divisor, max_dn, 4, compression, predictor


def wrap_image(samples, H=8, W=130):
    """Rows that hold 0, 65535, 1, 32768, 32767 next to each other (each row starts at another of them), the same in every channel
    shifted by one: the differences wrap both ways."""
    idx = (np.arange(W)[None, :, None] + np.arange(H)[:, None, None] + np.arange(samples)[None, None, :]) % 5
    img = WRAP[idx]
    return img[:, :, 0] if samples == 1 else img


def tie_values_u16(d, max_dn):
    """Samples v with (v / d) * max_dn exactly k + 0.5 for up to 4096 values of k spread over 0 .. max_dn - 1: the candidates
    (k + 0.5) / max_dn * d and their float neighbours."""
    k = np.unique(np.linspace(0, max_dn - 1, min(max_dn, 4096)).astype(np.int64)).astype(np.float64)
    c = (k + 0.5) / max_dn * d
    up, down = np.nextafter(c, np.inf), np.nextafter(c, -np.inf)
    cand = np.concatenate([c, up, down, np.nextafter(up, np.inf), np.nextafter(down, -np.inf)])
    prod = (cand / d) * max_dn
    return cand[(prod - np.floor(prod)) == 0.5]


def quantise_image_u16(d, max_dn, seed=0):
    """A (H, 64, 3) float64 image for divisor d: exact ties, 0, 1 / max_dn, d itself, and random values in [0, d]."""
    ties = tie_values_u16(d, max_dn)
    rng = np.random.default_rng(seed)
    v = np.concatenate([ties, [0.0, 1.0, d, d / max_dn], rng.random(4000) * d])
    v = np.resize(v, (-(-v.size // 192)) * 192)
    return v.reshape(-1, 64, 3), ties.size


def odd_row(max_dn):
    img = np.array([[np.nan, np.inf, -np.inf, -1.0 / max_dn, 0.0, 1.0, (max_dn + 1.0) / max_dn, 1e300]], dtype=np.float64)
    return img, [0, 0, 0, 65535, 0, max_dn, (max_dn + 1) % 65536, 0]


def narrowing_vectors():
    """A (H, 64) float64 image: doubles across the float32 normal range, doubles in the float32 subnormal range, +-1e39, exact ties
    between neighbouring float32 values (normal, subnormal and at the top of the range), +-0, +-inf and NaN."""
    rng = np.random.default_rng(17)
    normal = rng.standard_normal(3000) * 10.0 ** rng.uniform(-37, 38, 3000)
    tiny = 2.0 ** -149
    sub = np.concatenate([rng.uniform(-1, 1, 1000) * 2.0 ** -126, tiny * np.array([0.5, 0.5000001, 1.0, 1.5, 2.5, -0.5, -1.5, 0.25, 0.75])])
    f = np.concatenate([rng.standard_normal(500).astype(np.float32), (rng.uniform(-1, 1, 200) * 2.0 ** -127).astype(np.float32),
                        np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max], dtype=np.float32)])
    with np.errstate(over="ignore"):
        nxt = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    nxt[-2] = 2.0 ** 128                                           # above float32's largest: the tie rounds to the even one, inf
    ties = (f.astype(np.float64) + nxt) / 2                        # exact in float64: 25 bits
    edge = np.array([1e39, -1e39, 0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, 2.0 ** -126, 2.0 ** -127])
    v = np.concatenate([normal, sub, ties, edge])
    v = np.resize(v, (-(-v.size // 64)) * 64)
    return v.reshape(-1, 64), ties.size


def assert_narrowed(bits, img):
    """bits: the stored uint32 words; equal to astype(np.float32)'s for everything but NaN, a NaN for NaN."""
    with np.errstate(over="ignore"):
        want = img.astype(np.float32)
    nan = np.isnan(img)
    got = bits.view(np.float32).reshape(img.shape)
    assert np.isnan(got[nan]).all()
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    sub = (want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)
    assert sub.sum() >= 500 and np.isinf(want[~nan]).sum() >= 4    # the vectors do hold what the test is about


def host():
    from camera_linearity_amd import _native as nat
    return nat.host_lib()


# ---------------------------------------------------------------------------------------------------------------------
# 1. streams
# ---------------------------------------------------------------------------------------------------------------------
def test_host_build_strips_equal_the_numpy_expectation_byte_for_byte():
    lib = host()
    n_cases = 0
    for name, img, kind, divisor, max_dn, rps, compression, predictor in strip_cases():
        payload, offsets, counts, rc = abi_encode_wide(lib, img, kind, divisor, max_dn, rps, compression, predictor)
        assert rc == 0, name
        check_against_reference(img, kind, divisor, max_dn, rps, compression, predictor, payload, offsets, counts, lib)
        n_cases += 1
    assert n_cases == 5 * 3 * 2 * (2 + 1 + 1 + 2)                   # widths x samples x compressions x (kind, predictor) pairs


# ---------------------------------------------------------------------------------------------------------------------
# 2. the predictor where differences wrap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [1, 3, 4])
def test_predictor_differences_wrap_and_restart_with_every_row(samples):
    lib = host()
    img = wrap_image(samples)
    payload, offsets, counts, rc = abi_encode_wide(lib, img, U16, 1.0, 0, 4, 1, 2)           # two strips of four rows
    assert rc == 0
    check_against_reference(img, U16, 1.0, 0, 4, 1, 2, payload, offsets, counts, lib)
    stored = payload.view("<u2").reshape(8, 130, samples)
    file_order = bgr(img.reshape(8, 130, samples))
    assert np.array_equal(stored[:, 0], file_order[:, 0])                                    # first pixel of every row, inside a strip too
    assert np.array_equal(stored[:, 64], file_order[:, 64] - file_order[:, 63])              # the lane step does not restart the differences
    # 0 -> 65535 and 32768 -> 32767 are -1 = 65535, 65535 -> 1 is 2, 1 -> 32768 is 32767, 32767 -> 0 is -32767 = 32769
    assert set(np.unique(stored[:, 1:]).tolist()) == {2, 32767, 32769, 65535}
    payload5, offsets5, counts5, rc = abi_encode_wide(lib, img, U16, 1.0, 0, 4, 5, 2)
    assert rc == 0
    check_against_reference(img, U16, 1.0, 0, 4, 5, 2, payload5, offsets5, counts5, lib)


# ---------------------------------------------------------------------------------------------------------------------
# 3. kind 3: float64 -> uint16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_dn", [511, 4095, 65535])
@pytest.mark.parametrize("d", [1.0, 3.7])
def test_quantisation_is_save_16bit_arithmetic_with_ties(d, max_dn):
    img, n_ties = quantise_image_u16(d, max_dn)
    print(f"divisor {d}, max_dn {max_dn}: {n_ties} exact ties")
    assert n_ties >= 200
    payload, _, _, rc = abi_encode_wide(host(), img, F64_AS_U16, d, max_dn, 4, 1, 1)
    assert rc == 0
    want = np.mod(np.around((img / d) * max_dn), 65536).astype(np.uint16)
    assert np.array_equal(payload.view("<u2").reshape(img.shape), bgr(want))


@pytest.mark.parametrize("max_dn", [511, 4095, 65535])
def test_quantisation_of_non_finite_negative_and_huge_samples(max_dn):
    img, want = odd_row(max_dn)
    payload, _, _, rc = abi_encode_wide(host(), img, F64_AS_U16, 1.0, max_dn, 1, 1, 1)
    assert rc == 0
    assert list(payload.view("<u2")) == want


# ---------------------------------------------------------------------------------------------------------------------
# 4. kind 2: float64 -> float32
# ---------------------------------------------------------------------------------------------------------------------
def test_narrowing_is_astype_float32_bit_for_bit():
    img, n_ties = narrowing_vectors()
    assert n_ties >= 700
    payload, _, _, rc = abi_encode_wide(host(), img, F64_AS_F32, 1.0, 0, 4, 1, 1)
    assert rc == 0
    assert_narrowed(payload.view("<u4"), img)


# ---------------------------------------------------------------------------------------------------------------------
# 5. files
# ---------------------------------------------------------------------------------------------------------------------
def file_images(H=11):
    for W in WIDTHS:
        for samples in (1, 3, 4):
            yield f"u2s{samples}w{W}", source_image(U16, H, W, samples, seed=W + samples)
        for samples in (1, 3):
            yield f"f4s{samples}w{W}", source_image(F32, H, W, samples, seed=W + samples)


def file_options(img):
    """(compression, predictor) pairs hm_tiff_encode_strips_wide writes for the dtype."""
    return ((1, 1), (1, 2), (5, 1), (5, 2)) if img.dtype == np.uint16 else ((1, 1), (5, 1))


def test_imwrite_wide_files_read_back(tmp_path):
    n = 0
    for name, img in file_images():
        for compression, predictor in file_options(img):
            p = tmp_path / f"{name}.tif"
            assert T.imwrite(p, img, compression=compression, predictor=predictor, wide_samples=True)
            lay = T._parse_layout(memoryview(p.read_bytes()))
            assert (lay.compression, lay.predictor, lay.dtype) == (compression, predictor, img.dtype)
            got = T.imread(p, T.IMREAD_UNCHANGED)
            assert got.dtype == img.dtype and np.array_equal(got, img), (name, compression, predictor)
            n += 1
    assert n == 5 * (3 * 4 + 2 * 2)
    img = source_image(U16, 300, 129, 3, seed=1)                      # several rows per strip and a short last strip
    p = tmp_path / "tall.tif"
    T.imwrite(p, img, compression=5, predictor=2, wide_samples=True)
    assert T._parse_layout(memoryview(p.read_bytes())).rows_per_strip > 1
    assert np.array_equal(T.imread(p, T.IMREAD_UNCHANGED), img)


def pillow_samples(path, Image):
    """A several-sample LZW file without a predictor as Pillow / libtiff decode its strips, in FILE order: Pillow holds no mode for three
    16-bit or float samples, so the strips are handed to it under a uint8 IFD - same strip bytes, offsets, counts and compression, the
    width times the sample size - and the bytes it decodes are viewed as the file's samples (pillow_array of
    tests/test_tiff_encode_host.py does this for float64)."""
    buf = path.read_bytes()
    lay = T._parse_layout(memoryview(buf))
    assert lay.compression == 5 and lay.predictor == 1
    H, W, S = lay.shape
    n = lay.n_strips
    total = lay.offsets[n - 1] - 8 + -(-lay.counts[n - 1] // 16) * 16
    head, tail = T._file_frame(H, W * lay.dtype.itemsize, S, np.dtype(np.uint8), lay.rows_per_strip, [o - 8 for o in lay.offsets[:n]],
                               lay.counts[:n], total, 5, 1)
    as_bytes = path.with_suffix(".u8.tif")
    as_bytes.write_bytes(head + buf[8:8 + total] + tail)
    with Image.open(as_bytes) as im:
        raw = np.ascontiguousarray(np.asarray(im)).reshape(-1)
    return raw.view(lay.dtype).reshape(H, W, S)


def test_imwrite_wide_files_read_by_pillow(tmp_path):
    """Pillow / libtiff read one-sample uint16 (I;16) and float32 (F) files as they are: uint16 LZW + Predictor 2 and float32 LZW. They
    hold no mode for three 16-bit or float samples: the LZW strips of those files are decoded by libtiff under a uint8 IFD
    (pillow_samples), which a 16-bit predictor does not allow, so several-sample Predictor 2 files are checked by imread above."""
    Image = pytest.importorskip("PIL.Image")
    n = 0
    for name, img in file_images():
        p = tmp_path / f"{name}.tif"
        if img.ndim == 2:
            T.imwrite(p, img, compression=5, predictor=2 if img.dtype == np.uint16 else 1, wide_samples=True)
            with Image.open(p) as im:
                got = np.asarray(im)
            assert got.dtype == img.dtype and np.array_equal(got, img), name
        else:
            T.imwrite(p, img, compression=5, wide_samples=True)
            got = pillow_samples(p, Image)
            assert got.dtype == img.dtype and np.array_equal(got, bgr(img)), name
        n += 1
    assert n == 25


def test_the_keyword_alone_changes_no_byte(tmp_path):
    for name, img in file_images():
        T.imwrite(tmp_path / "a.tif", img)
        T.imwrite(tmp_path / "b.tif", img, compression=1, predictor=1, wide_samples=True)
        assert (tmp_path / "a.tif").read_bytes() == (tmp_path / "b.tif").read_bytes(), name
    for img in (np.arange(60, dtype=np.uint8).reshape(4, 5, 3), np.random.default_rng(1).random((4, 5, 3))):
        for kw in (dict(), dict(compression=5)):
            T.imwrite(tmp_path / "a.tif", img, **kw)
            T.imwrite(tmp_path / "b.tif", img, wide_samples=True, **kw)
            assert (tmp_path / "a.tif").read_bytes() == (tmp_path / "b.tif").read_bytes()


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_encode_strips_wide_rejects_bad_arguments_in_the_stated_order():
    """Every check of hm_tiff_encode_strips_wide returns before any HIP call, so none of these touches a GPU (there is none here) or
    dereferences a pointer: the pointers below are made-up addresses. Where two rules are broken, the earlier one answers."""
    from camera_linearity_amd import _native as nat
    P = 1 << 20                                  # never dereferenced
    good = dict(src=P, kind=U16, div=1.0, max_dn=0, h=4, w=8, s=3, rps=1, comp=5, pred=1, payload=P, cap=1 << 20, offs=P, cnts=P, ws=P)
    for lib in (nat.hip_lib, nat.host_lib()):
        def call(**kw):
            a = dict(good, **kw)
            return lib.hm_tiff_encode_strips_wide(a["src"], a["kind"], a["div"], a["max_dn"], a["h"], a["w"], a["s"], a["rps"], a["comp"],
                                                  a["pred"], a["payload"], a["cap"], a["offs"], a["cnts"], a["ws"], None)
        # HM_EINVAL: pointers, sizes, predictor
        for null in ("src", "payload", "offs", "cnts"):
            assert call(**{null: None}) == nat.HM_EINVAL, null
            assert call(**{null: None}, comp=8) == nat.HM_EINVAL, null
        for name in ("h", "w", "rps"):
            assert call(**{name: 0}) == nat.HM_EINVAL and call(**{name: -1}) == nat.HM_EINVAL, name
            assert call(**{name: 0}, s=2) == nat.HM_EINVAL, name
        assert call(pred=0) == nat.HM_EINVAL and call(pred=3) == nat.HM_EINVAL and call(pred=3, kind=9) == nat.HM_EINVAL
        # HM_EINVAL: kind 3's divisor and max_dn, the workspace of Compression 5 - read for kind 3 only
        for d in (0.0, -1.0, float("nan"), float("inf")):
            assert call(kind=F64_AS_U16, max_dn=4095, div=d) == nat.HM_EINVAL, d
            assert call(kind=F64_AS_U16, max_dn=4095, div=d, comp=8) == nat.HM_EINVAL, d
            for kind in (U16, F32, F64_AS_F32):
                assert call(kind=kind, div=d, max_dn=-1, comp=8) == nat.HM_EUNSUPPORTED, (kind, d)      # not EINVAL: not read
        for m in (0, -1, 65536, 1 << 20):
            assert call(kind=F64_AS_U16, max_dn=m) == nat.HM_EINVAL, m
            assert call(kind=F64_AS_U16, max_dn=m, s=5) == nat.HM_EINVAL, m
        assert call(ws=None) == nat.HM_EINVAL and call(ws=None, s=2) == nat.HM_EINVAL
        assert call(ws=None, comp=1, cap=0) == nat.HM_ESHAPE                          # not EINVAL: Compression 1 needs no workspace
        # HM_EUNSUPPORTED: compression, samples, kind, Predictor 2 with float32 output
        for comp in (0, 8, 32773, 32946):
            assert call(comp=comp) == nat.HM_EUNSUPPORTED, comp
            assert call(comp=comp, cap=0, payload=P + 8) == nat.HM_EUNSUPPORTED, comp
        for s in (0, 2, 5):
            assert call(s=s) == nat.HM_EUNSUPPORTED and call(s=s, cap=0) == nat.HM_EUNSUPPORTED, s
        assert call(kind=4) == nat.HM_EUNSUPPORTED and call(kind=-1) == nat.HM_EUNSUPPORTED and call(kind=4, cap=0) == nat.HM_EUNSUPPORTED
        for kind in (F32, F64_AS_F32):
            assert call(kind=kind, pred=2) == nat.HM_EUNSUPPORTED and call(kind=kind, pred=2, src=P + 2, cap=0) == nat.HM_EUNSUPPORTED
        # HM_ESHAPE: the strip size, payload_cap
        need = lib.hm_tiff_encode_payload_bytes(4, 48, 5)
        assert call(cap=need - 1) == nat.HM_ESHAPE and call(cap=0) == nat.HM_ESHAPE and call(cap=-1) == nat.HM_ESHAPE
        assert call(cap=need - 1, payload=P + 8) == nat.HM_ESHAPE
        assert call(comp=1, cap=4 * 48 - 1) == nat.HM_ESHAPE
        assert call(h=2, rps=2, w=1 << 29, s=4, cap=1 << 62) == nat.HM_ESHAPE           # strips of 2^32 bytes
        assert call(h=1, w=(1 << 30), s=1, cap=1 << 62) == nat.HM_ESHAPE                # exactly 2^31
        assert call(h=1, w=(1 << 29), s=1, kind=F32, cap=1 << 62) == nat.HM_ESHAPE      # exactly 2^31
        # HM_EALIGN: payload and workspace to 16, tables to 8, the source to its own sample
        assert call(payload=P + 8) == nat.HM_EALIGN and call(ws=P + 4) == nat.HM_EALIGN
        assert call(offs=P + 4) == nat.HM_EALIGN and call(cnts=P + 4) == nat.HM_EALIGN
        assert call(kind=U16, src=P + 1) == nat.HM_EALIGN and call(kind=F32, src=P + 2) == nat.HM_EALIGN
        assert call(kind=F64_AS_F32, src=P + 4) == nat.HM_EALIGN and call(kind=F64_AS_U16, max_dn=4095, src=P + 4) == nat.HM_EALIGN
    import torch
    if not torch.cuda.is_available():            # valid arguments meet no device
        call = nat.hip_lib.hm_tiff_encode_strips_wide
        assert call(P, U16, 1.0, 0, 4, 8, 3, 1, 5, 2, P, 1 << 20, P, P, P, None) == nat.HM_ELAUNCH
        assert call(P + 2, U16, 1.0, 0, 4, 8, 3, 1, 1, 1, P, 1 << 20, P, P, None, None) == nat.HM_ELAUNCH
        assert call(P, F64_AS_U16, 2.0, 4095, 4, 8, 3, 1, 1, 2, P, 1 << 20, P, P, None, None) == nat.HM_ELAUNCH


def test_imwrite_refusals_without_the_keyword_are_unchanged(tmp_path):
    f = np.random.default_rng(4).random((4, 5, 3))
    u = np.arange(60, dtype=np.uint8).reshape(4, 5, 3)
    p = tmp_path / "no.tif"
    for img, kw in ((f, dict(predictor=2)), (f, dict(compression=5, predictor=2)), (u, dict(compression=8)), (u, dict(compression=32773)),
                    (u, dict(predictor=3)), (u.astype(np.uint16), dict(compression=5)), (f.astype(np.float32), dict(compression=5)),
                    (u.astype(np.uint16), dict(predictor=2)), (u.astype(np.uint16), dict(compression=5, predictor=2))):
        with pytest.raises((ValueError, NotImplementedError)):
            T.imwrite(p, img, **kw)
        assert not p.exists(), kw
    # with it: what hm_tiff_encode_strips_wide does not write is still refused before the file exists
    for img, kw in ((f, dict(predictor=2)), (f.astype(np.float32), dict(predictor=2)), (f.astype(np.float32), dict(compression=5, predictor=2)),
                    (u.astype(np.uint16), dict(compression=8)), (u.astype(np.uint16), dict(predictor=3))):
        with pytest.raises((ValueError, NotImplementedError)):
            T.imwrite(p, img, wide_samples=True, **kw)
        assert not p.exists(), kw


def test_imwrite_device_wide_refuses_host_tensors_before_any_launch(tmp_path):
    import torch
    from camera_linearity_amd import _native as nat
    before = nat.hip_lib.calls["hm_tiff_encode_strips_wide"]
    for t, kw in ((torch.zeros((4, 5, 3), dtype=torch.uint16), dict(wide_samples=True)),
                  (torch.zeros((4, 5, 3), dtype=torch.float32), dict(wide_samples=True)),
                  (torch.zeros((4, 5, 3), dtype=torch.float64), dict(narrow_to_float32=True)),
                  (torch.zeros((4, 5, 3), dtype=torch.float64), dict(quantize_divisor=1.0, quantize_max_dn=4095)),
                  (np.zeros((4, 5, 3), dtype=np.uint16), dict(wide_samples=True))):
        with pytest.raises((ValueError, TypeError)):
            T.imwrite_device(tmp_path / "h.tif", t, **kw)
    assert nat.hip_lib.calls["hm_tiff_encode_strips_wide"] == before and not (tmp_path / "h.tif").exists()


# ---------------------------------------------------------------------------------------------------------------------
# 7. ImageSet on the host backend
# ---------------------------------------------------------------------------------------------------------------------
def merged_arrays():
    """A 24 x 20 x 3 'merged' image with values above 1 (so save_16bit scales) and a std image with values above 1 too."""
    rng = np.random.default_rng(33)
    val = rng.random((24, 20, 3)) * 5.0 + np.add.outer(np.arange(24), np.arange(20))[:, :, None] / 20.0
    std = rng.random((24, 20, 3)) * 1.5
    return val, std


@pytest.mark.parametrize("force_16_bit", [False, True])
@pytest.mark.parametrize("bit_depth,compression,predictor", [(16, 1, 1), (12, 5, 2), (10, 1, 2)])
def test_save_16bit_on_the_host_backend(tmp_path, bit_depth, compression, predictor, force_16_bit):
    from camera_linearity_amd.image_set import ImageSet
    val, std = merged_arrays()
    s = ImageSet(file_path=tmp_path / "10ms bf 5x merged.tif", value=val, std=std, use_cupy=False)
    s.save_16bit(bit_depth=bit_depth, compression=compression, predictor=predictor, force_16_bit=force_16_bit)
    folder = tmp_path / "16bit"
    assert sorted(p.name for p in folder.glob("*")) == ["10ms bf 5x merged STD.tif", "10ms bf 5x merged.tif"]
    max_dn = 2 ** bit_depth - 1
    got = T.imread(folder / "10ms bf 5x merged.tif", T.IMREAD_UNCHANGED)
    assert got.dtype == np.uint16 and got.max() == max_dn
    assert np.array_equal(got, np.around((val / val.max()) * max_dn).astype(np.uint16))
    lay = T._parse_layout(memoryview((folder / "10ms bf 5x merged.tif").read_bytes()))
    assert (lay.compression, lay.predictor) == (compression, predictor)
    got_std = T.imread(folder / "10ms bf 5x merged STD.tif", T.IMREAD_UNCHANGED)
    if force_16_bit:
        assert got_std.dtype == np.uint16 and np.array_equal(got_std, np.around((std / std.max()) * max_dn).astype(np.uint16))
    else:
        assert got_std.dtype == np.float64 and np.array_equal(got_std, std)
    small = ImageSet(file_path=tmp_path / "10ms bf 5x small.tif", value=val / 10.0, use_cupy=False)      # maximum below 1: no scaling
    small.save_16bit(tmp_path / "s.tif", bit_depth=bit_depth)
    assert np.array_equal(T.imread(tmp_path / "s.tif", T.IMREAD_UNCHANGED), np.around((val / 10.0) * max_dn).astype(np.uint16))
    with pytest.raises(ValueError, match="device backend"):
        s.save_16bit(tmp_path / "d.tif", device_encode=True)
    with pytest.raises(ValueError, match="bit_depth"):
        s.save_16bit(tmp_path / "d.tif", bit_depth=17)
    assert not (tmp_path / "d.tif").exists()


def test_save_32bit_on_the_host_backend(tmp_path):
    from camera_linearity_amd.image_set import ImageSet
    val, std = merged_arrays()
    s = ImageSet(file_path=tmp_path / "10ms bf 5x merged.tif", value=val, std=std, use_cupy=False)
    s.save_32bit(is_HDR=True)
    folder = tmp_path / "32bit"
    assert sorted(p.name for p in folder.glob("*")) == ["10ms bf 5x merged HDR STD.tif", "10ms bf 5x merged HDR.tif"]
    got = T.imread(folder / "10ms bf 5x merged HDR.tif", T.IMREAD_UNCHANGED)
    assert got.dtype == np.float32 and np.array_equal(got, val.astype(np.float32))
    got = T.imread(folder / "10ms bf 5x merged HDR STD.tif", T.IMREAD_UNCHANGED)
    assert got.dtype == np.float32 and np.array_equal(got, std.astype(np.float32))
    with pytest.raises(ValueError, match="device backend"):
        s.save_32bit(tmp_path / "d.tif", device_encode=True)
    assert not (tmp_path / "d.tif").exists()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the row text under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_body_header_under_asan_and_ubsan(tmp_path):
    """tools/tiff_wide_enc_body_check.cpp, a stand-alone executable: csrc/hm_tiff_wide_enc_body.h over the test shapes with heap blocks
    of exactly the row's bytes, under AddressSanitizer and UBSan on the CPU. Nothing is loaded into this process."""
    exe = tmp_path / "tiff_wide_enc_body_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           f"-I{ROOT / 'camera_linearity_amd' / 'csrc'}", str(ROOT / "tools" / "tiff_wide_enc_body_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal to the reference" in r.stdout
