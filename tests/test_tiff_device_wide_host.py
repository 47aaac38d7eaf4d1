"""The wide device TIFF path (tiff_io.imread_device(wide_samples=True), hm_tiff_decode_strips_wide: uint16, float32 and big-endian
multi-byte samples) as far as a box without a GPU can check it, and the helpers its GPU tests share
(tests/test_gpu_tiff_device_wide.py).

Here: the argument rules of the entry in both libraries, which return before any HIP call; the wide file family through the host
build's entry against tiff_io.imread, byte for byte; short and damaged strips on the host build; and imread_device's remaining
refusals, decided from the IFD before the GPU is touched. Files come from the writer of tests/test_tiff_device_host.py."""
import numpy as np
import pytest

from camera_linearity_amd import tiff_io as T

from test_tiff_device_host import bgr, lzw_encode, pack_codes, write_tiff


# ---------------------------------------------------------------------------------------------------------------------
# helpers (shared with tests/test_gpu_tiff_device_wide.py)
# ---------------------------------------------------------------------------------------------------------------------
# widths below, at and past one wave step (64 pixels) and past two; a one-pixel column; one row of 3000 pixels, which with 3 samples
# is 18 000 bytes: past the 16 KiB a wave decodes in LDS
SHAPES = [(5, 1), (3, 63), (3, 64), (3, 65), (4, 129), (33, 47)]
LONG_SHAPE = (2, 3000)


def wide_image(shape, samples, seed):
    """family_image widened to 16 bits: the left half a smooth ramp whose step (0x0203 per pixel, 0x0303 per row) moves both bytes, the
    right half noise over the whole range."""
    H, W = shape
    rng = np.random.default_rng(seed)
    img = (np.add.outer(np.arange(H) * 0x0303, np.arange(W) * 0x0203)[:, :, None] + np.arange(samples) * 10280 + 0x1234) % 65536
    img = img.astype(np.uint16)
    noisy = rng.integers(0, 65536, img.shape, dtype=np.uint16)
    img[:, W // 2:] = noisy[:, W // 2:]
    return img[:, :, 0] if samples == 1 else img


def assert_u16_image_exercises_the_row_pass(a):
    """What makes a wrong decode show: both bytes of the horizontal differences are in use, the running sums of a row pass 65536 (so the
    carry must wrap), and the top byte differs from the bottom one and varies (so `>> 8` and a byte-order mistake both change values).
    The first two need a row to sum over: they are asserted from 47 pixels on (the one-pixel column has no difference at all)."""
    a3 = a[:, :, None] if a.ndim == 2 else a
    hi, lo = a3 >> 8, a3 & 0xFF
    assert len(np.unique(hi)) > 1 and (hi != lo).any()
    if a3.shape[1] >= 47:
        d = (a3[:, 1:].astype(np.int64) - a3[:, :-1]) % 65536
        assert ((d & 0xFF) != 0).any() and ((d >> 8) != 0).any()
        assert (a3.astype(np.int64).sum(axis=1) > 65535).all()


def float_image(shape, samples, dtype, seed):
    """Finite floats of both signs and many exponents: every byte of a sample varies."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(shape + (samples,)) * 10.0 ** rng.integers(-3, 4, shape + (samples,))).astype(dtype)
    return a[:, :, 0] if samples == 1 else a


def wide_family(dtype, compression, predictor, byteorder):
    """One (sample type, compression, predictor, byte order): samples x shape x rows per strip -> (name, array, write_tiff keywords).
    Uncompressed files start their first strip at offset 9, so every strip lies at an odd offset for 3 samples and at offsets that are
    no multiple of the sample size for the rest."""
    dtype = np.dtype(dtype)
    kw = dict(compression=compression, predictor=predictor, byteorder=byteorder)
    for samples in ((1, 3, 4) if dtype.kind == "u" else (1, 3)):
        cases = [(shape, rps) for shape in SHAPES for rps in dict.fromkeys((1, 3, shape[0]))]
        if samples == 3:
            cases.append((LONG_SHAPE, 1))
        for shape, rps in cases:
            seed = shape[0] * 7 + shape[1] + samples
            img = wide_image(shape, samples, seed) if dtype.kind == "u" else float_image(shape, samples, dtype, seed)
            name = f"{dtype.name}{'le' if byteorder == '<' else 'be'}_c{compression}p{predictor}s{samples}_{shape[0]}x{shape[1]}_r{rps}.tif"
            yield name, img, dict(kw, rows_per_strip=rps)
            if compression == 1:
                yield "odd_" + name, img, dict(kw, rows_per_strip=rps, first_offset=9)


U16_KINDS = [(c, p, bo) for c in (1, 5) for p in (1, 2) for bo in "<>"]
FLOAT_KINDS = [(np.float32, c, bo) for c in (1, 5) for bo in "<>"] + [(np.float64, c, ">") for c in (1, 5)]


def flags_of(dtype):
    return (T.IMREAD_COLOR, T.IMREAD_UNCHANGED) if np.dtype(dtype).kind == "u" else (T.IMREAD_UNCHANGED,)


def abi_read_wide(lib, path, flag):
    """A file through hm_tiff_decode_strips_wide of `lib` with HOST arrays (the host build): (frame, status)."""
    buf = np.fromfile(path, dtype=np.uint8)
    lay = T._parse_layout(memoryview(buf))
    H, W, S = lay.shape
    n, bps = lay.n_strips, lay.dtype.itemsize
    offs = np.array(lay.offsets[:n], dtype=np.int64)
    cnts = np.array(lay.counts[:n], dtype=np.int64)
    ws = np.empty(max(1, lib.hm_tiff_decode_workspace_bytes(n, lay.rows_per_strip * lay.row_bytes, lay.compression)), dtype=np.uint8)
    status = np.full(n, -99, dtype=np.int64)
    color = flag == T.IMREAD_COLOR
    out_s = 3 if color else S
    dst = np.zeros((H, W) if out_s == 1 else (H, W, out_s), dtype=np.uint8 if color else lay.dtype.newbyteorder("="))
    rc = lib.hm_tiff_decode_strips_wide(buf.ctypes.data, buf.size, offs.ctypes.data, cnts.ctypes.data, n, lay.compression, lay.predictor,
                                        lay.rows_per_strip, H, W, S, bps, int(lay.dtype.byteorder == ">"), int(color), dst.ctypes.data,
                                        status.ctypes.data, ws.ctypes.data, None)
    assert rc == 0
    return dst, status


CANARY = 0xA5
FILL = 0xEE          # what dst holds before a call: a byte the call did not write still shows it


def damaged_cases():
    """Fixed inputs the decoder refuses or cuts short by design, as raw calls: name -> dict(blob, offs, cnts, file_len, comp, pred, H, W,
    S, bps, be, color, plain). One row per strip throughout; `plain` is the file-order uint16 image the intact strips hold."""
    out = {}
    W = 10
    rgb = wide_image((3, W), 3, seed=5)
    rgba = wide_image((3, W), 4, seed=6)
    for name, img, extra in (("short_1", rgb, 1), ("short_3", rgb, 3), ("short_7", rgb, 7), ("short_rgba_7", rgba, 7)):
        S = img.shape[2]
        row = W * S * 2
        blob = img.astype("<u2").tobytes()
        cut = 4 * S * 2 + extra                                       # strip 1 ends `extra` bytes past its fourth pixel
        out[name] = dict(blob=blob, offs=[0, row, 2 * row], cnts=[row, cut, row], file_len=len(blob), comp=1, pred=1, H=3, W=W, S=S,
                         bps=2, be=0, color=0, plain=img)
    # the same cut in a big-endian Predictor 2 file read as 8-bit colour: the scan stops with the pixels
    stored = rgb.copy()
    stored[:, 1:] = rgb[:, 1:] - rgb[:, :-1]
    blob = stored.astype(">u2").tobytes()
    row = W * 6
    out["short_be_p2_color"] = dict(blob=blob, offs=[0, row, 2 * row], cnts=[row, 4 * 6 + 5, row], file_len=len(blob), comp=1, pred=2,
                                    H=3, W=W, S=3, bps=2, be=1, color=1, plain=rgb)
    # LZW: strip 1 holds an invalid code (300 > next), strip 3 lies beyond the end of the file
    img = wide_image((5, 40), 3, seed=7)
    streams = [lzw_encode(img[r].astype("<u2").tobytes()) for r in range(5)]
    streams[1] = pack_codes([256, 65, 300, 257])
    offs = np.cumsum([0] + [len(s) for s in streams[:-1]])
    cnts = np.array([len(s) for s in streams])
    file_len = int(offs[-1] + cnts[-1])
    offs[3], cnts[3] = file_len - 10, 100
    out["lzw_corrupt_and_beyond"] = dict(blob=b"".join(streams), offs=list(offs), cnts=list(cnts), file_len=file_len, comp=5, pred=1, H=5,
                                         W=40, S=3, bps=2, be=0, color=0, plain=img)
    # uncompressed: strip 2 lies beyond the end of the file
    img = wide_image((4, 8), 1, seed=8)[:, :, None]
    blob = img.astype("<u2").tobytes()
    out["raw_beyond"] = dict(blob=blob, offs=[0, 16, 60, 48], cnts=[16, 16, 16, 16], file_len=64, comp=1, pred=1, H=4, W=8, S=1, bps=2,
                             be=0, color=0, plain=img)
    return out


def out_row_bytes(case):
    return case["W"] * (3 if case["color"] else case["S"] * case["bps"])


def host_wide_call(lib, case):
    """The raw call of a damaged_cases() entry on HOST arrays: (status, dst rows as bytes (H, out_row_bytes), canaries intact)."""
    n = case["H"]
    blob = np.frombuffer(case["blob"] + bytes(8), dtype=np.uint8).copy()
    offs, cnts = np.array(case["offs"], dtype=np.int64), np.array(case["cnts"], dtype=np.int64)
    rb = out_row_bytes(case)
    dst = np.full(64 + n * rb + 64, CANARY, dtype=np.uint8)
    dst[64:64 + n * rb] = FILL
    status = np.full(n, -99, dtype=np.int64)
    ws = np.empty(max(1, lib.hm_tiff_decode_workspace_bytes(n, case["W"] * case["S"] * case["bps"], case["comp"])), dtype=np.uint8)
    rc = lib.hm_tiff_decode_strips_wide(blob.ctypes.data, case["file_len"], offs.ctypes.data, cnts.ctypes.data, n, case["comp"], case["pred"],
                                        1, n, case["W"], case["S"], case["bps"], case["be"], case["color"], dst.ctypes.data + 64,
                                        status.ctypes.data, ws.ctypes.data, None)
    assert rc == 0
    ok = bool((dst[:64] == CANARY).all() and (dst[64 + n * rb:] == CANARY).all())
    return status, dst[64:64 + n * rb].reshape(n, rb).copy(), ok


def expected_rows(case):
    """What imread would give for the intact image of a damaged_cases() entry, as bytes per row."""
    want = bgr(case["plain"])
    if case["color"]:
        want = (want >> 8).astype(np.uint8)[:, :, :3]
    return np.ascontiguousarray(want).view(np.uint8).reshape(case["H"], -1)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["device build", "host build"])
def test_decode_strips_wide_rejects_bad_arguments_without_a_device(which):
    """Every check of hm_tiff_decode_strips_wide returns before any HIP call and before any pointer is read: the pointers are made-up
    addresses, and every call below breaks at least one rule (a call that breaks none would launch)."""
    from camera_linearity_amd import _native as nat
    fn = (nat.hip_lib if which == "device build" else nat.host_lib()).hm_tiff_decode_strips_wide
    P = 4096                                     # never dereferenced
    good = dict(file=P, file_len=100, offs=P, cnts=P, n=4, comp=5, pred=1, rps=1, h=4, w=8, s=3, b=2, be=0, color=0, dst=P, st=P, ws=P)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["file"], a["file_len"], a["offs"], a["cnts"], a["n"], a["comp"], a["pred"], a["rps"], a["h"], a["w"], a["s"], a["b"],
                  a["be"], a["color"], a["dst"], a["st"], a["ws"], None)
    for null in ("file", "offs", "cnts", "dst", "st", "ws"):
        assert call(**{null: None}) == nat.HM_EINVAL, null
    assert call(file_len=-1) == nat.HM_EINVAL
    assert call(n=0) == nat.HM_EINVAL and call(rps=0) == nat.HM_EINVAL and call(h=0) == nat.HM_EINVAL and call(w=0) == nat.HM_EINVAL
    assert call(pred=3) == nat.HM_EINVAL and call(color=2) == nat.HM_EINVAL
    assert call(be=2) == nat.HM_EINVAL and call(be=-1) == nat.HM_EINVAL
    for comp in (0, 8, 32773, 32946):
        assert call(comp=comp) == nat.HM_EUNSUPPORTED, comp
    for s in (0, 2, 5):
        assert call(s=s) == nat.HM_EUNSUPPORTED, s
    for b in (1, 3, 16):                         # 1-byte samples belong to hm_tiff_decode_strips
        assert call(b=b) == nat.HM_EUNSUPPORTED, b
    for b in (4, 8):
        assert call(b=b, pred=2) == nat.HM_EUNSUPPORTED, b            # the predictor exists for 2-byte samples
        assert call(b=b, color=1) == nat.HM_EUNSUPPORTED, b           # and so does the 8-bit conversion
    assert call(n=3) == nat.HM_ESHAPE and call(n=5) == nat.HM_ESHAPE  # 4 rows, 1 per strip: 4 strips
    assert call(rps=3, n=4) == nat.HM_ESHAPE
    assert call(h=2, rps=2, n=1, w=1 << 30, s=4, b=2) == nat.HM_ESHAPE     # strips past 2^31 bytes
    assert call(h=2, rps=2, n=1, w=1 << 30, s=1, b=8) == nat.HM_ESHAPE
    assert call(dst=P + 1) == nat.HM_EALIGN
    assert call(b=4, dst=P + 2) == nat.HM_EALIGN and call(b=8, dst=P + 4) == nat.HM_EALIGN
    # two broken rules: the earlier code wins - EINVAL, EUNSUPPORTED, ESHAPE, EALIGN
    assert call(be=2, b=3) == nat.HM_EINVAL
    assert call(file=None, dst=P + 1) == nat.HM_EINVAL
    assert call(ws=None, n=3) == nat.HM_EINVAL
    assert call(b=3, n=3) == nat.HM_EUNSUPPORTED
    assert call(b=4, pred=2, dst=P + 1) == nat.HM_EUNSUPPORTED
    assert call(n=3, dst=P + 1) == nat.HM_ESHAPE


# ---------------------------------------------------------------------------------------------------------------------
# the file family through the host build
# ---------------------------------------------------------------------------------------------------------------------
def check_family_on_the_host_build(tmp_path, dtype, compression, predictor, byteorder):
    from camera_linearity_amd import _native as nat
    n = 0
    for name, img, kw in wide_family(dtype, compression, predictor, byteorder):
        if np.dtype(dtype).kind == "u":
            assert_u16_image_exercises_the_row_pass(img)
        p = tmp_path / name
        write_tiff(p, img, **kw)
        for flag in flags_of(dtype):
            got, status = abi_read_wide(nat.host_lib(), p, flag)
            want = T.imread(p, flag)
            assert got.dtype == want.dtype and got.shape == want.shape, (name, flag)
            assert got.tobytes() == want.tobytes(), (name, flag)
            assert (status > 0).all()
        n += 1
    assert n >= 31                                                        # 15 (shape, rows per strip) pairs per sample count + the long row


@pytest.mark.parametrize("compression,predictor,byteorder", U16_KINDS)
def test_host_build_decodes_the_uint16_family(tmp_path, compression, predictor, byteorder):
    check_family_on_the_host_build(tmp_path, np.uint16, compression, predictor, byteorder)


@pytest.mark.parametrize("dtype,compression,byteorder", FLOAT_KINDS)
def test_host_build_decodes_the_float_family(tmp_path, dtype, compression, byteorder):
    check_family_on_the_host_build(tmp_path, dtype, compression, 1, byteorder)


def test_long_row_and_images_are_what_the_cases_need():
    """The 3000-pixel row is past the 16 KiB LDS stage and its running sums wrap 65536 many hundred times."""
    img = wide_image(LONG_SHAPE, 3, seed=1)
    assert img[0].nbytes == 18000 > 16 * 1024
    assert (img.astype(np.int64).sum(axis=1) > 500 * 65536).all()
    assert_u16_image_exercises_the_row_pass(img)


# ---------------------------------------------------------------------------------------------------------------------
# short and damaged strips on the host build
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["short_1", "short_3", "short_7", "short_rgba_7", "short_be_p2_color"])
def test_short_strip_fills_whole_pixels_only(name):
    from camera_linearity_amd import _native as nat
    case = damaged_cases()[name]
    status, rows, ok = host_wide_call(nat.host_lib(), case)
    want = expected_rows(case)
    px_in, px_out = case["S"] * case["bps"], out_row_bytes(case) // case["W"]
    whole = case["cnts"][1] // px_in
    assert 0 < whole < case["W"] and case["cnts"][1] % px_in != 0       # the count ends inside a pixel
    assert list(status) == case["cnts"]                                 # the status is the count
    assert np.array_equal(rows[[0, 2]], want[[0, 2]])
    assert np.array_equal(rows[1, :whole * px_out], want[1, :whole * px_out])
    assert (rows[1, whole * px_out:] == FILL).all()                     # nothing of the cut pixel, nothing behind it
    assert ok


def test_damaged_strips_leave_their_rows_and_their_neighbours_alone():
    from camera_linearity_amd import _native as nat
    cases = damaged_cases()
    case = cases["lzw_corrupt_and_beyond"]
    status, rows, ok = host_wide_call(nat.host_lib(), case)
    full = case["W"] * 6
    assert list(status) == [full, nat.HM_EINVAL, full, nat.HM_EINVAL, full]
    want = expected_rows(case)
    assert np.array_equal(rows[[0, 2, 4]], want[[0, 2, 4]])
    assert (rows[[1, 3]] == FILL).all() and ok
    case = cases["raw_beyond"]
    status, rows, ok = host_wide_call(nat.host_lib(), case)
    assert list(status) == [16, 16, nat.HM_EINVAL, 16]
    want = expected_rows(case)
    assert np.array_equal(rows[[0, 1, 3]], want[[0, 1, 3]]) and (rows[2] == FILL).all() and ok


# ---------------------------------------------------------------------------------------------------------------------
# Python without a GPU: what wide_samples=True still refuses, from the IFD
# ---------------------------------------------------------------------------------------------------------------------
def test_wide_samples_still_refuses_from_the_ifd(tmp_path):
    u16 = wide_image((8, 9), 3, seed=4)
    f32 = float_image((8, 9), 3, np.float32, seed=5)
    files = {
        "deflate": (u16, dict(compression=8)),
        "packbits": (u16, dict(compression=32773)),
        "tiles": (u16, dict(extra_tags=[(322, 3, [16]), (323, 3, [16]), (324, 4, [8]), (325, 4, [16 * 16 * 6])])),
        "int16": (u16.astype(np.int16), {}),
        "predictor_on_float32": (f32, dict(extra_tags=[(317, 3, [2])])),             # the tag only: no reader here undoes a float predictor
        "white_is_zero": (u16[:, :, 0], dict(extra_tags=[(262, 3, [0])])),           # a second PhotometricInterpretation: the last one counts
    }
    for name, (a, kw) in files.items():
        p = tmp_path / f"{name}.tif"
        write_tiff(p, a, **kw)
        for flag in (T.IMREAD_UNCHANGED, T.IMREAD_COLOR):
            with pytest.raises(NotImplementedError, match=r"tiff_io\.imread"):
                T.imread_device(p, flag, wide_samples=True)
            with pytest.raises(NotImplementedError, match=r"tiff_io\.imread"):
                T.DeviceTiffReader().read(p, flag, wide_samples=True)
    assert T._parse_layout(memoryview((tmp_path / "white_is_zero.tif").read_bytes())).photometric == 0
    p = tmp_path / "f32.tif"
    write_tiff(p, f32, byteorder=">")
    with pytest.raises(NotImplementedError, match=r"tiff_io\.imread"):                # floats -> 8 bits stays on the host
        T.imread_device(p, T.IMREAD_COLOR, wide_samples=True)
    T._device_layout_check(T._parse_layout(memoryview(p.read_bytes())), T.IMREAD_UNCHANGED, wide_samples=True)      # accepted
    with pytest.raises(NotImplementedError, match=r"tiff_io\.imread"):                # and without the keyword nothing has changed
        T.imread_device(p, T.IMREAD_UNCHANGED)
    assert T.imread_device(tmp_path / "absent.tif", wide_samples=True) is None
    assert T.DeviceTiffReader().read(tmp_path / "absent.tif", T.IMREAD_UNCHANGED, wide_samples=True) is None
