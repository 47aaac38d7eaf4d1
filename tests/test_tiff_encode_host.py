"""The TIFF writing path (hm_tiff_encode_strips, tiff_io.imwrite(compression=5), imwrite_device's refusals) as far as a box without a
GPU can check it, and the helpers its GPU tests share (tests/test_gpu_tiff_encode.py).

The host build's hm_tiff_encode_strips runs the encoder body both builds share, so every strip is pinned here against lzw_encode of
tests/test_tiff_device_host.py - the project's statement of the stream format - byte for byte; the GPU tests then compare the device
call with the host build's. Also here: the size bound, the uint8 quantisation with exact ties, files read back by imread and Pillow,
the unchanged default file, the argument validation (it returns before any HIP call) and device_encode=True on a host-backend ImageSet."""
import hashlib
import itertools

import numpy as np
import pytest

from camera_linearity_amd import tiff_io as T
from test_tiff_device_host import bgr, family_image, lzw_encode


# ---------------------------------------------------------------------------------------------------------------------
# helpers (shared with tests/test_gpu_tiff_encode.py)
# ---------------------------------------------------------------------------------------------------------------------
def data_kinds(n, seed=0):
    """The four kinds of strip content the bound was examined on: zeros, a ramp, noise, and byte pairs that do not repeat."""
    rng = np.random.default_rng(seed + n)
    k = np.arange(n, dtype=np.int64)
    return {
        "zeros": np.zeros(n, dtype=np.uint8),
        "ramp": (k % 256).astype(np.uint8),
        "noise": rng.integers(0, 256, n, dtype=np.uint8),
        "pairs": ((k + (k // 256) * (k % 256)) % 256).astype(np.uint8),        # stride k // 256 + 1: every (a, a + stride) pair is new
    }


def packed_reference(img, kind, divisor, predictor):
    """What the pack step must produce for a BGR(A) array: file order, quantised for kind 2, Predictor 2 applied."""
    a = np.asarray(img)
    a3 = a[:, :, None] if a.ndim == 2 else a
    if kind == 2:
        with np.errstate(invalid="ignore", over="ignore"):
            a3 = np.around((a3 / divisor) * 255.0).astype(np.uint8)
    f = bgr(a3) if a3.shape[2] >= 3 else a3
    if predictor == 2:
        g = f.copy()
        g[:, 1:] = f[:, 1:] - f[:, :-1]
        f = g
    return np.ascontiguousarray(f)


def abi_encode(lib, img, kind=0, divisor=1.0, rows_per_strip=1, compression=5, predictor=1, on_device=False):
    """A BGR(A) array through hm_tiff_encode_strips of `lib`: (payload[:total], offsets, counts, rc). Host arrays for the host build;
    with on_device the arrays are torch tensors on the GPU with 4 KiB of 0xA5 behind payload and workspace, which must survive."""
    a = np.ascontiguousarray(img)
    a3 = a[:, :, None] if a.ndim == 2 else a
    H, W, S = a3.shape
    rps = min(rows_per_strip, H)
    n = -(-H // rps)
    strip_bytes = rps * W * S * (8 if kind == 1 else 1)
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
        rc = lib.hm_tiff_encode_strips(src.data_ptr(), kind, divisor, H, W, S, rows_per_strip, compression, predictor, payload.data_ptr(), cap,
                                       tables.data_ptr(), tables.data_ptr() + 8 * (n + 1), ws.data_ptr() if wsb else None,
                                       nat.current_stream_ptr(dev))
        torch.cuda.synchronize()
        payload, ws, tables = payload.cpu().numpy(), ws.cpu().numpy(), tables.cpu().numpy()
        assert (payload[cap:] == 0xA5).all() and (ws[max(wsb, 16):] == 0xA5).all(), "a byte behind the stated sizes was written"
        offsets, counts = tables[:n + 1], tables[n + 1:]
    else:
        payload = np.full(cap, 0xA5, dtype=np.uint8)
        ws = np.full(max(wsb, 16), 0xA5, dtype=np.uint8)
        offsets = np.full(n + 1, -99, dtype=np.int64)
        counts = np.full(n, -99, dtype=np.int64)
        rc = lib.hm_tiff_encode_strips(a.ctypes.data, kind, divisor, H, W, S, rows_per_strip, compression, predictor, payload.ctypes.data, cap,
                                       offsets.ctypes.data, counts.ctypes.data, ws.ctypes.data if wsb else None, None)
    if rc != 0:
        return None, offsets, counts, rc
    total = int(offsets[n])
    assert 0 <= total <= cap
    return payload[:total].copy(), offsets.copy(), counts.copy(), rc


def check_against_lzw_encode(img, kind, divisor, rows_per_strip, predictor, payload, offsets, counts, lib):
    """Every strip equals lzw_encode of the packed, predicted strip; offsets are multiples of 16, counts exact, gaps zero, last = total."""
    ref = packed_reference(img, kind, divisor, predictor)
    H = ref.shape[0]
    rps = min(rows_per_strip, H)
    n = -(-H // rps)
    pos = 0
    for s in range(n):
        raw = ref[s * rps:(s + 1) * rps].tobytes()
        want = lzw_encode(raw)
        assert offsets[s] == pos and pos % 16 == 0, (s, offsets[s], pos)
        assert counts[s] == len(want), (s, counts[s], len(want))
        assert len(want) <= lib.hm_tiff_encode_bound(len(raw))
        assert payload[pos:pos + len(want)].tobytes() == want, s
        end = -(-(pos + len(want)) // 16) * 16
        assert not payload[pos + len(want):end].any(), f"gap after strip {s} is not zero"
        pos = end
    assert offsets[n] == pos == len(payload)


def first_clear(data: np.ndarray) -> int:
    """The smallest n for which lzw_encode(data[:n]) holds a Clear after the first (the table filled up), 0 if none does."""
    def clears(n):
        st = {}
        lzw_encode(data[:n].tobytes(), stats=st)
        return st["clears"]
    if clears(len(data)) == 0:
        return 0
    lo, hi = 1, len(data)
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if clears(mid) else (mid + 1, hi)
    return lo


def strip_cases():
    """(name, BGR(A) array, kind, rows_per_strip, predictor): strip sizes 1, 2, 3, 255, 256, just below, at and above the first Clear
    of each data kind that reaches one, 12 288 and 98 304 of the four data kinds as one-row grey strips; 3- and 4-sample images with
    both predictors and a short last strip; a 1 x 1 image; float64 and quantised strips."""
    sizes = {name: [1, 2, 3, 255, 256, 12288, 98304] for name in data_kinds(1)}
    for name, data in data_kinds(12288).items():
        n = first_clear(data)
        if n:
            sizes[name] += [n - 1, n, n + 1]
    assert len(sizes["noise"]) == 10 and len(sizes["pairs"]) == 10
    for name, ns in sizes.items():
        for n in ns:
            yield f"{name}{n}", data_kinds(12288 if n < 12288 else n)[name][:n].reshape(1, n), 0, 1, 1
    for samples, (H, W), rps, predictor in itertools.product((1, 3, 4), ((1, 1), (7, 5), (37, 101)), (1, 3, 5), (1, 2)):
        yield f"img{samples}_{H}x{W}_r{rps}_p{predictor}", family_image((H, W), samples, seed=H + samples), 0, rps, predictor
    f = np.random.default_rng(5).random((7, 9, 3))
    yield "f64_r2", f, 1, 2, 1
    yield "f64_rows_of_12288", np.random.default_rng(6).random((2, 512, 3)), 1, 1, 1           # a float64 row: 12 288 bytes
    yield "quantised_r3_p2", f * 3.0, 2, 3, 2


def tie_values(d):
    """Samples v with (v / d) * 255.0 exactly k + 0.5, k = 0..255: the candidates (k + 0.5) / 255 * d and their float neighbours."""
    k = np.arange(256, dtype=np.float64)
    c = (k + 0.5) / 255.0 * d
    cand = np.concatenate([c, np.nextafter(c, np.inf), np.nextafter(c, -np.inf), np.nextafter(np.nextafter(c, np.inf), np.inf),
                           np.nextafter(np.nextafter(c, -np.inf), -np.inf)])
    prod = (cand / d) * 255.0
    return cand[(prod - np.floor(prod)) == 0.5]


def quantise_image(d, seed=0):
    """A (H, 64, 3) float64 image for divisor d: exact ties, 0, 1 / 255, d itself, and random values in [0, d]."""
    ties = tie_values(d)
    rng = np.random.default_rng(seed)
    v = np.concatenate([ties, [0.0, 1.0, d, d / 255.0], rng.random(4000) * d])
    v = np.resize(v, (-(-v.size // 192)) * 192)
    return v.reshape(-1, 64, 3), ties.size


# ---------------------------------------------------------------------------------------------------------------------
# 1. streams
# ---------------------------------------------------------------------------------------------------------------------
def test_host_build_streams_equal_lzw_encode_byte_for_byte():
    from camera_linearity_amd import _native as nat
    lib = nat.host_lib()
    n_cases = 0
    for name, img, kind, rps, predictor in strip_cases():
        divisor = 3.0 if kind == 2 else 1.0
        payload, offsets, counts, rc = abi_encode(lib, img, kind, divisor, rps, 5, predictor)
        assert rc == 0, name
        check_against_lzw_encode(img, kind, divisor, rps, predictor, payload, offsets, counts, lib)
        n_cases += 1
    assert n_cases > 80


def test_uncompressed_payload_is_the_packed_image():
    from camera_linearity_amd import _native as nat
    lib = nat.host_lib()
    for samples, predictor, rps in itertools.product((1, 3, 4), (1, 2), (1, 4, 100)):
        img = family_image((9, 13), samples, seed=samples)
        payload, offsets, counts, rc = abi_encode(lib, img, 0, 1.0, rps, 1, predictor)
        assert rc == 0
        ref = packed_reference(img, 0, 1.0, predictor)
        assert payload.tobytes() == ref.tobytes()
        r = min(rps, 9)
        n = -(-9 // r)
        row = 13 * samples
        assert list(offsets) == [s * r * row for s in range(n)] + [9 * row]
        assert list(counts) == [row * min(r, 9 - s * r) for s in range(n)]
    f = np.random.default_rng(2).random((5, 7, 3))
    payload, _, _, rc = abi_encode(lib, f, 1, 1.0, 2, 1, 1)
    assert rc == 0 and payload.tobytes() == bgr(f).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the bound
# ---------------------------------------------------------------------------------------------------------------------
def test_encode_bound_holds_and_is_tight():
    from camera_linearity_amd import _native as nat
    for lib in (nat.host_lib(), nat.hip_lib):
        for n in (1, 2, 3, 255, 256, 3836, 3837, 4096, 12288, 98304):
            assert lib.hm_tiff_encode_bound(n) == (3 * n + 1) // 2 + n // 2048 + 8
        for n in (0, -1, 1 << 31, 1 << 62):
            assert lib.hm_tiff_encode_bound(n) < 0, n
            for fn in (lib.hm_tiff_encode_workspace_bytes, lib.hm_tiff_encode_payload_bytes):
                assert fn(4, n, 5) == 0, n
        for fn in (lib.hm_tiff_encode_workspace_bytes, lib.hm_tiff_encode_payload_bytes):
            assert fn(0, 100, 5) == 0 and fn(-1, 100, 5) == 0 and fn(4, 100, 8) == 0
        assert lib.hm_tiff_encode_workspace_bytes(4, 100, 1) == 0 and lib.hm_tiff_encode_payload_bytes(4, 100, 1) == 400
        b = (lib.hm_tiff_encode_bound(100) + 15) // 16 * 16
        assert lib.hm_tiff_encode_payload_bytes(4, 100, 5) == 4 * b and lib.hm_tiff_encode_workspace_bytes(4, 100, 5) == 4 * (112 + b)
        big = lib.hm_tiff_encode_workspace_bytes((1 << 31) - 1, (1 << 31) - 1, 5)
        assert big > (1 << 62)                                        # the largest geometry: the product is exact, not wrapped
    lib = nat.host_lib()
    noise = data_kinds(98304)["noise"].reshape(1, -1)
    _, _, counts, rc = abi_encode(lib, noise, 0, 1.0, 1, 5, 1)
    ratio = counts[0] / lib.hm_tiff_encode_bound(98304)
    print(f"noise of 98 304 bytes: {counts[0]} bytes, {ratio:.3f} of the bound")
    assert rc == 0 and 0.85 <= ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 3. quantisation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1.0, 2.0, 3.7, 255.0])
def test_quantisation_is_save_8bit_arithmetic_with_ties(d):
    from camera_linearity_amd import _native as nat
    img, n_ties = quantise_image(d)
    print(f"divisor {d}: {n_ties} exact ties")
    assert n_ties >= 200
    payload, _, _, rc = abi_encode(nat.host_lib(), img, 2, d, 4, 1, 1)
    assert rc == 0
    want = np.around((img / d) * 255.0).astype(np.uint8)
    assert np.array_equal(payload.reshape(img.shape), bgr(want))


def test_quantisation_of_non_finite_and_negative_samples():
    from camera_linearity_amd import _native as nat
    img = np.array([[np.nan, np.inf, -np.inf, -1.0 / 255.0, 0.0, 1.0, 256.0 / 255.0, 1e300]], dtype=np.float64)
    payload, _, _, rc = abi_encode(nat.host_lib(), img, 2, 1.0, 1, 1, 1)
    assert rc == 0
    assert list(payload) == [0, 0, 0, 255, 0, 255, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# 4. files
# ---------------------------------------------------------------------------------------------------------------------
def file_images():
    rng = np.random.default_rng(8)
    for W in (1, 63, 64, 65, 129):
        for samples in (1, 3, 4):
            yield f"u8s{samples}w{W}", family_image((11, W), samples, seed=W + samples)
        for samples in (1, 3):
            f = rng.random((11, W, samples)) * 4.0
            yield f"f8s{samples}w{W}", f[:, :, 0] if samples == 1 else f


@pytest.mark.parametrize("predictor", [1, 2])
def test_imwrite_lzw_files_read_back(tmp_path, predictor):
    for name, img in file_images():
        if img.dtype != np.uint8 and predictor == 2:
            continue
        p = tmp_path / f"{name}.tif"
        assert T.imwrite(p, img, compression=5, predictor=predictor)
        lay = T._parse_layout(memoryview(p.read_bytes()))
        assert (lay.compression, lay.predictor) == (5, predictor)
        got = T.imread(p, T.IMREAD_UNCHANGED)
        assert got.dtype == img.dtype and np.array_equal(got, img), name
        if img.dtype == np.uint8:
            col = T.imread(p)
            want = np.repeat(img[:, :, None], 3, axis=2) if img.ndim == 2 else img[:, :, :3]
            assert np.array_equal(col, want), name
    img = family_image((300, 129), 3, seed=1)                         # more than one row per strip and a short last strip
    p = tmp_path / "tall.tif"
    T.imwrite(p, img, compression=5, predictor=predictor)
    assert np.array_equal(T.imread(p, T.IMREAD_UNCHANGED), img)
    p1 = tmp_path / "tall_p.tif"
    T.imwrite(p1, img, compression=1, predictor=predictor)            # the predictor without compression
    assert np.array_equal(T.imread(p1, T.IMREAD_UNCHANGED), img)


def pillow_array(path):
    """The file as Pillow / libtiff decodes it, in FILE order. Pillow has no 64-bit float mode (its mode table holds no 64-bit entry, and
    it does not identify the uncompressed float64 files of imwrite either), so a float64 file's strips are handed to it under a uint8
    IFD - same strip bytes, offsets, counts and compression, eight times the width - and the bytes it decodes are viewed as float64."""
    from PIL import Image
    buf = path.read_bytes()
    lay = T._parse_layout(memoryview(buf))
    if lay.dtype == np.uint8:
        with Image.open(path) as im:
            return np.asarray(im)
    H, W, S = lay.shape
    n = lay.n_strips
    total = lay.offsets[n - 1] - 8 + -(-lay.counts[n - 1] // 16) * 16 if lay.compression == 5 else H * lay.row_bytes
    head, tail = T._file_frame(H, W * 8, S, np.dtype(np.uint8), lay.rows_per_strip, [o - 8 for o in lay.offsets[:n]], lay.counts[:n], total,
                               lay.compression, lay.predictor)
    as_bytes = path.with_suffix(".u8.tif")
    as_bytes.write_bytes(head + buf[8:8 + total] + tail)
    with Image.open(as_bytes) as im:
        raw = np.ascontiguousarray(np.asarray(im)).reshape(-1)
    return raw.view("<f8").reshape((H, W) if S == 1 else (H, W, S))


@pytest.mark.parametrize("predictor", [1, 2])
def test_imwrite_lzw_files_read_by_pillow(tmp_path, predictor):
    pytest.importorskip("PIL.Image")
    n = 0
    for name, img in file_images():
        if img.dtype != np.uint8 and predictor == 2:
            continue
        p = tmp_path / f"{name}.tif"
        T.imwrite(p, img, compression=5, predictor=predictor)
        got = pillow_array(p)
        want = bgr(img)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
        n += 1
    assert n == (25 if predictor == 1 else 15)


def test_imwrite_refuses_before_the_file_exists(tmp_path):
    f = np.random.default_rng(4).random((4, 5, 3))
    u = family_image((4, 5), 3, seed=1)
    for img, kw in ((f, dict(predictor=2)), (f, dict(compression=5, predictor=2)), (u, dict(compression=8)), (u, dict(compression=32773)),
                    (u, dict(predictor=3)), (u.astype(np.uint16), dict(compression=5)), (f.astype(np.float32), dict(compression=5)),
                    (u.astype(np.uint16), dict(predictor=2))):
        p = tmp_path / "no.tif"
        with pytest.raises((ValueError, NotImplementedError)):
            T.imwrite(p, img, **kw)
        assert not p.exists(), kw


def test_default_imwrite_file_is_unchanged(tmp_path):
    """SHA-256 of the files the commit before this feature wrote for the same arrays."""
    rng = np.random.default_rng(2024)
    u8 = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    f8 = rng.random((5, 7, 3))
    for name, a, sha in (("u8", u8, "01c8d72887fc89980649959d393ff3f20e16d6a417c9562b53d81db9f3c26ad7"),
                         ("f8", f8, "11132fea24754dd0d7f6a9335103e9e1c072ffeedf52fd3c84c33dc6ff4affad")):
        p = tmp_path / f"{name}.tif"
        T.imwrite(p, a)
        assert hashlib.sha256(p.read_bytes()).hexdigest() == sha, name
        q = tmp_path / f"{name}_kw.tif"
        T.imwrite(q, a, compression=1, predictor=1)
        assert q.read_bytes() == p.read_bytes()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
def test_encode_strips_rejects_bad_arguments_without_a_device():
    """Every check of hm_tiff_encode_strips returns before any HIP call, so none of these touches a GPU (there is none here) or
    dereferences a pointer: the pointers below are made-up addresses."""
    from camera_linearity_amd import _native as nat
    P = 1 << 20                                  # never dereferenced
    good = dict(src=P, kind=0, div=1.0, h=4, w=8, s=3, rps=1, comp=5, pred=1, payload=P, cap=1 << 20, offs=P, cnts=P, ws=P)
    for lib in (nat.hip_lib, nat.host_lib()):
        def call(**kw):
            a = dict(good, **kw)
            return lib.hm_tiff_encode_strips(a["src"], a["kind"], a["div"], a["h"], a["w"], a["s"], a["rps"], a["comp"], a["pred"],
                                             a["payload"], a["cap"], a["offs"], a["cnts"], a["ws"], None)
        for null in ("src", "payload", "offs", "cnts", "ws"):
            assert call(**{null: None}) == nat.HM_EINVAL, null
        for name in ("h", "w", "rps"):
            assert call(**{name: 0}) == nat.HM_EINVAL and call(**{name: -1}) == nat.HM_EINVAL, name
        for d in (0.0, -1.0, float("nan"), float("inf")):
            assert call(kind=2, div=d) == nat.HM_EINVAL, d
        assert call(pred=0) == nat.HM_EINVAL and call(pred=3) == nat.HM_EINVAL
        for comp in (0, 8, 32773, 32946):
            assert call(comp=comp) == nat.HM_EUNSUPPORTED, comp
        for s in (0, 2, 5):
            assert call(s=s) == nat.HM_EUNSUPPORTED, s
        assert call(kind=3) == nat.HM_EUNSUPPORTED and call(kind=-1) == nat.HM_EUNSUPPORTED
        assert call(kind=1, pred=2) == nat.HM_EUNSUPPORTED            # predictor 2 with 8-byte output
        need = lib.hm_tiff_encode_payload_bytes(4, 24, 5)
        assert call(cap=need - 1) == nat.HM_ESHAPE and call(cap=0) == nat.HM_ESHAPE and call(cap=-1) == nat.HM_ESHAPE
        assert call(comp=1, cap=95) == nat.HM_ESHAPE
        assert call(h=2, rps=2, w=1 << 30, s=4, cap=1 << 62) == nat.HM_ESHAPE        # strips of 2^31 bytes or more
        assert call(h=1, w=(1 << 28), s=1, kind=1, cap=1 << 62) == nat.HM_ESHAPE     # exactly 2^31
        assert call(payload=P + 8) == nat.HM_EALIGN and call(ws=P + 4) == nat.HM_EALIGN and call(kind=1, src=P + 4) == nat.HM_EALIGN
    call = nat.hip_lib.hm_tiff_encode_strips                          # valid arguments meet no device
    import torch
    if not torch.cuda.is_available():
        assert call(P, 0, 1.0, 4, 8, 3, 1, 5, 1, P, 1 << 20, P, P, P, None) == nat.HM_ELAUNCH
        assert call(P, 2, 2.0, 4, 8, 3, 1, 1, 2, P, 1 << 20, P, P, None, None) == nat.HM_ELAUNCH


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals of the Python layer that need no GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_device_encode_needs_the_device_backend(tmp_path):
    from camera_linearity_amd.image_set import ImageSet
    p = tmp_path / "10ms bf 5x thing.tif"
    T.imwrite(p, family_image((8, 9), 3, seed=7))
    s = ImageSet(file_path=p, use_cupy=False)
    s.load_value_image()
    with pytest.raises(ValueError, match="device backend"):
        s.save_64bit(tmp_path / "o64.tif", device_encode=True)
    with pytest.raises(ValueError, match="device backend"):
        s.save_8bit(tmp_path / "o8.tif", device_encode=True)
    assert not (tmp_path / "o64.tif").exists() and not (tmp_path / "o8.tif").exists()
    s.save_8bit(tmp_path / "o8.tif")                                  # the default path is untouched
    assert np.array_equal(T.imread(tmp_path / "o8.tif", T.IMREAD_UNCHANGED), family_image((8, 9), 3, seed=7))


def test_imwrite_device_refuses_host_tensors_before_any_launch(tmp_path):
    import torch
    from camera_linearity_amd import _native as nat
    before = nat.hip_lib.calls["hm_tiff_encode_strips"]
    with pytest.raises((ValueError, TypeError)):
        T.imwrite_device(tmp_path / "h.tif", torch.zeros((4, 5, 3), dtype=torch.uint8))
    with pytest.raises((ValueError, TypeError)):
        T.imwrite_device(tmp_path / "h.tif", np.zeros((4, 5, 3), dtype=np.uint8))
    assert nat.hip_lib.calls["hm_tiff_encode_strips"] == before and not (tmp_path / "h.tif").exists()
