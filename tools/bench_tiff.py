#!/usr/bin/env python3
"""TIFF read throughput: 4096 x 4096 x 3 uint8 images - uncompressed, and LZW as OpenCV / libtiff write it (via PIL when it is
installed) for a smooth, a photo-like (gradient + sensor noise) and a noise image; float64 uncompressed. Pixel MB/s, second read of each file.

Without arguments: the host path (tiff_io.imread) only, no GPU needed. `--device`: the device path (tiff_io.imread_device) next to it, on
the same files in the same run - timed from the open() of the file to the synchronised status read-back, so the upload of the file's
bytes is inside - and the wall time of `ExposureSeries.from_dir_path -> load_value_images -> process_HDR_image` for a stack of
7 x 4096 x 4096 x 3 LZW frames both ways (warm: the second run of each). Then the wide samples (`imread_device(wide_samples=True)`,
hm_tiff_decode_strips_wide) on 4096 x 4096 x 3 files, host `imread` against the device in the same run: uint16 with 12-bit content,
photo-like and noise, LZW + Predictor 2 and uncompressed; float32 uncompressed; a big-endian uint16 uncompressed file; and loading a
7-frame 12-bit LZW stack plus `engine.merge(bit_depth=12)` through both decoders. `--wide-only` (with `--device`) runs only these.

`--write` (needs a GPU; nothing else runs): the way out of HBM. For a smooth, a photo-like and a noise image of 4096 x 4096 x 3 and
2048 x 2048 x 3 held by a device-backend ImageSet as a float64 value image (values up to 4) with a std image, the wall time from the
device-resident image to the closed files of `save_8bit` (compression 1 and 5) and `save_64bit` (val and std), host path against
`device_encode=True`, warm (the median of three runs after a first, with the fastest and slowest in brackets), the size of the value file, and the device time of hm_tiff_encode_strips alone
(HIP events around the call) with compression 1 - the pack kernel only - and 5, whose difference is the LZW kernel with its scan and
compaction. The host path is the code of the commit before the device writer, unchanged, so one run gives both sides.

`--device --wide-write` (needs a GPU; nothing else runs): the wide samples on the way out, 4096 x 4096 x 3 images resident in device
memory, host path against `imwrite_device` in one run, pixel MB/s of the stored image (median of five warm runs after a first, fastest
and slowest in brackets): uint16 with 12-bit content, photo-like and noise, LZW + Predictor 2; uint16 uncompressed; float32 uncompressed;
float64 stored as float32; float64 quantised to 12 bits, LZW + Predictor 2. The host column is the copy to the host, the NumPy
conversion where there is one and `imwrite(wide_samples=True)` - for uncompressed float32 the only path there was - with `imwrite` alone
(array already on the host) beside it; the device column is `imwrite_device` with `wide_samples`, `narrow_to_float32` or
`quantize_max_dn`. The two files are compared byte for byte. Last, the device time of hm_tiff_encode_strips_wide alone (HIP events)."""
import argparse
import pathlib
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from camera_linearity_amd import tiff_io as T  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--device", action="store_true", help="also time tiff_io.imread_device and the 7-frame load-and-merge both ways (needs a GPU)")
ap.add_argument("--write", action="store_true", help="time ImageSet.save_8bit / save_64bit, host path against device_encode=True (needs a GPU)")
ap.add_argument("--wide-only", action="store_true", help="with --device: only the rows of the wide samples (uint16, float32, big-endian)")
ap.add_argument("--wide-write", action="store_true", help="with --device: only the writing rows of the wide samples, imwrite(wide_samples=True) "
                                                          "against imwrite_device (uint16, float32, float64 narrowed / quantised)")
args = ap.parse_args()


def bench_write():
    import shutil
    import torch
    from camera_linearity_amd import _native as nat
    from camera_linearity_amd.image_set import ImageSet
    d = pathlib.Path(tempfile.mkdtemp())
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)

    class Ms(float):
        """A median of three warm runs that prints with its spread."""
        def __format__(self, spec):
            return f"{float(self):{spec}} ({self.lo:.0f}-{self.hi:.0f})"

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) * 1e3)
        runs.sort()
        m = Ms(runs[1])
        m.lo, m.hi = runs[0], runs[2]
        return m

    def encode_ms(t, kind, divisor, compression, predictor=1):
        """Device time of one hm_tiff_encode_strips (HIP events), warm, best of 3."""
        H, W, S = t.shape
        row = W * S * (8 if kind == 1 else 1)
        rps = max(1, min(H, 8192 // row))
        n = -(-H // rps)
        lib = nat.hip_lib
        cap = lib.hm_tiff_encode_payload_bytes(n, rps * row, compression)
        payload = torch.empty(cap, dtype=torch.uint8, device=dev)
        ws = torch.empty(max(16, lib.hm_tiff_encode_workspace_bytes(n, rps * row, compression)), dtype=torch.uint8, device=dev)
        tables = torch.empty(2 * n + 1, dtype=torch.int64, device=dev)
        best = float("inf")
        for _ in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            nat.check(lib.hm_tiff_encode_strips(t.data_ptr(), kind, divisor, H, W, S, rps, compression, predictor, payload.data_ptr(), cap,
                                                tables.data_ptr(), tables.data_ptr() + 8 * (n + 1), ws.data_ptr(),
                                                nat.current_stream_ptr(dev)), "hm_tiff_encode_strips")
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        total = int(tables[n].item())
        return best, total

    for size in (4096, 2048):
        ramp = np.add.outer(np.arange(size), np.arange(size))[:, :, None]
        images = {"smooth": (ramp // 37 % 256 * np.ones(3)) / 255.0 * 4.0,
                  "photo-like": np.clip(ramp / 40 + rng.normal(size=(size, size, 3)) * 2, 0, 255) / 255.0 * 4.0,
                  "noise": rng.random((size, size, 3)) * 4.0}
        for name, val in images.items():
            std = np.ascontiguousarray(val[::-1]) * 0.01 + 1e-3
            s_ = ImageSet(file_path=d / "10ms bf 5x scene.tif", value=val, std=std, use_cupy=True)
            mb8, mb64 = val.size / 1e6, val.nbytes / 1e6
            print(f"--- {size} x {size} x 3, {name}: uint8 image {mb8:.0f} MB, float64 image {mb64:.0f} MB", flush=True)
            for compression in (1, 5):
                th = timed(lambda: s_.save_8bit(d / "h8.tif", compression=compression))
                td = timed(lambda: s_.save_8bit(d / "d8.tif", device_encode=True, compression=compression))
                a, b = T.imread(d / "h8.tif", T.IMREAD_UNCHANGED), T.imread(d / "d8.tif", T.IMREAD_UNCHANGED)
                assert np.array_equal(a, b)
                print(f"save_8bit (uint8 val + float64 std) compression {compression}: host {th:.0f} ms, device_encode {td:.0f} ms "
                      f"({float(th) / float(td):.1f} x), val file {(d / 'd8.tif').stat().st_size / 1e6:.1f} MB", flush=True)
            th = timed(lambda: s_.save_64bit(d / "h64.tif"))
            td = timed(lambda: s_.save_64bit(d / "d64.tif", device_encode=True))
            assert (d / "h64.tif").read_bytes() == (d / "d64.tif").read_bytes()
            print(f"save_64bit (val + std, uncompressed): host {th:.0f} ms, device_encode {td:.0f} ms ({float(th) / float(td):.1f} x)", flush=True)
            tv = s_.measurand.val
            hv = val
            th = timed(lambda: T.imwrite(d / "h64z.tif", hv, compression=5))
            td = timed(lambda: T.imwrite_device(d / "d64z.tif", tv, compression=5))
            assert (d / "h64z.tif").read_bytes() == (d / "d64z.tif").read_bytes()
            print(f"float64 val with LZW (array already on its side): imwrite {th:.0f} ms, imwrite_device {td:.0f} ms, "
                  f"file {(d / 'd64z.tif').stat().st_size / 1e6:.0f} MB against {mb64:.0f} MB uncompressed", flush=True)
            divisor = float(val.max())
            p1, _ = encode_ms(tv, 2, divisor, 1)
            p5, tot = encode_ms(tv, 2, divisor, 5)
            q5, tot2 = encode_ms(tv, 2, divisor, 5, predictor=2)
            f1, _ = encode_ms(tv, 1, 1.0, 1)
            f5, totf = encode_ms(tv, 1, 1.0, 5)
            print(f"hm_tiff_encode_strips alone: float64 -> uint8 pack {p1:.2f} ms, with LZW {p5:.2f} ms (LZW + scan + compaction "
                  f"{p5 - p1:.2f} ms, payload {tot / 1e6:.1f} MB; predictor 2: {q5:.2f} ms, {tot2 / 1e6:.1f} MB); float64 pack {f1:.2f} ms, "
                  f"with LZW {f5:.2f} ms (payload {totf / 1e6:.0f} MB)", flush=True)
            del s_, tv
    shutil.rmtree(d)


def bench_wide_write():
    import shutil
    import torch
    from camera_linearity_amd import _native as nat
    d = pathlib.Path(tempfile.mkdtemp())
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    size = 4096
    ramp = np.add.outer(np.arange(size), np.arange(size))[:, :, None]

    def timed(fn, reps=5):
        """(median, fastest, slowest) seconds of `reps` warm runs after a first."""
        fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        runs.sort()
        return runs[len(runs) // 2], runs[0], runs[-1]

    def rate(nbytes, t):
        return f"{nbytes / t[0] / 1e6:.0f} ({nbytes / t[2] / 1e6:.0f}-{nbytes / t[1] / 1e6:.0f}) MB/s"

    def encode_ms(t, kind, out_bytes, divisor, max_dn, compression, predictor):
        """Device time of one hm_tiff_encode_strips_wide (HIP events), warm: the median of five."""
        H, W, S = t.shape
        row = W * S * out_bytes
        rps = T._strip_rows(H, row)
        n = -(-H // rps)
        lib = nat.hip_lib
        cap = lib.hm_tiff_encode_payload_bytes(n, rps * row, compression)
        payload = torch.empty(cap, dtype=torch.uint8, device=dev)
        ws = torch.empty(max(16, lib.hm_tiff_encode_workspace_bytes(n, rps * row, compression)), dtype=torch.uint8, device=dev)
        tables = torch.empty(2 * n + 1, dtype=torch.int64, device=dev)
        times = []
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            nat.check(lib.hm_tiff_encode_strips_wide(t.data_ptr(), kind, divisor, max_dn, H, W, S, rps, compression, predictor,
                                                     payload.data_ptr(), cap, tables.data_ptr(), tables.data_ptr() + 8 * (n + 1),
                                                     ws.data_ptr(), nat.current_stream_ptr(dev)), "hm_tiff_encode_strips_wide")
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return sorted(times[1:])[2]

    def row(name, tensor, to_host, stored_bytes, host_kw, dev_kw, abi):
        """One line: the host path from the device tensor (copy down, `to_host` conversion, imwrite), imwrite alone, imwrite_device."""
        host_img = to_host(tensor.cpu().numpy())
        th = timed(lambda: T.imwrite(d / "h.tif", to_host(tensor.cpu().numpy()), wide_samples=True, **host_kw))
        ta = timed(lambda: T.imwrite(d / "h.tif", host_img, wide_samples=True, **host_kw))
        td = timed(lambda: T.imwrite_device(d / "d.tif", tensor, **dev_kw, **host_kw))
        assert (d / "h.tif").read_bytes() == (d / "d.tif").read_bytes(), name
        ms = encode_ms(tensor, *abi, host_kw.get("compression", 1), host_kw.get("predictor", 1))
        moved = tensor.numel() * tensor.element_size() + stored_bytes
        print(f"{name}: host {rate(stored_bytes, th)} (imwrite alone {rate(stored_bytes, ta)}), device {rate(stored_bytes, td)} "
              f"({th[0] / td[0]:.1f} x); file {(d / 'd.tif').stat().st_size / 1e6:.1f} MB; hm_tiff_encode_strips_wide alone {ms:.2f} ms"
              + (f" = {moved / ms / 1e6:.0f} GB/s read + written" if host_kw.get("compression", 1) == 1 else ""), flush=True)

    def same(a):
        return a
    lzw2 = dict(compression=5, predictor=2)
    photo = np.clip(ramp * (4095 / 8190) + rng.normal(size=(size, size, 3)) * 8, 0, 4095).astype(np.uint16)
    noise = rng.integers(0, 4096, (size, size, 3), dtype=np.uint16)
    wide = dict(wide_samples=True)
    print(f"--- {size} x {size} x 3, pixel MB/s of the stored image, median (slowest-fastest) of 5 warm runs", flush=True)
    t = torch.from_numpy(photo).to(dev)
    row("uint16 12-bit photo-like, LZW + Predictor 2", t, same, photo.nbytes, lzw2, wide, (nat.HM_TIFF_SRC_U16, 2, 1.0, 0))
    row("uint16 uncompressed", t, same, photo.nbytes, {}, wide, (nat.HM_TIFF_SRC_U16, 2, 1.0, 0))
    t = torch.from_numpy(noise).to(dev)
    row("uint16 12-bit noise, LZW + Predictor 2", t, same, noise.nbytes, lzw2, wide, (nat.HM_TIFF_SRC_U16, 2, 1.0, 0))
    del noise
    f64 = photo / 4095.0 * 3.7
    del photo
    t = torch.from_numpy(f64.astype(np.float32)).to(dev)
    row("float32 uncompressed", t, same, f64.size * 4, {}, wide, (nat.HM_TIFF_SRC_F32, 4, 1.0, 0))
    t = torch.from_numpy(f64).to(dev)
    del f64
    row("float64 -> float32 uncompressed", t, lambda a: a.astype(np.float32), t.numel() * 4, {}, dict(narrow_to_float32=True),
        (nat.HM_TIFF_SRC_F64_AS_F32, 4, 1.0, 0))
    row("float64 -> 12-bit uint16, LZW + Predictor 2", t, lambda a: np.around((a / 3.7) * 4095).astype(np.uint16), t.numel() * 2, lzw2,
        dict(quantize_divisor=3.7, quantize_max_dn=4095), (nat.HM_TIFF_SRC_F64_AS_U16, 2, 3.7, 4095))
    shutil.rmtree(d)


if args.write:
    bench_write()
    sys.exit(0)
if args.wide_write:
    if not args.device:
        ap.error("--wide-write needs --device")
    bench_wide_write()
    sys.exit(0)

d = pathlib.Path(tempfile.mkdtemp())
rng = np.random.default_rng(0)
ramp = np.add.outer(np.arange(4096), np.arange(4096))[:, :, None]
images = {} if args.wide_only else {
    "smooth": (ramp // 37 % 256 * np.ones(3)).astype(np.uint8),
    "photo-like": np.clip(ramp / 40 + rng.normal(size=(4096, 4096, 3)) * 2, 0, 255).astype(np.uint8),
    "noise": (rng.random((4096, 4096, 3)) * 255).astype(np.uint8)}


def timed_read(path, flag=None):
    T.imread(path) if flag is None else T.imread(path, flag)
    t0 = time.perf_counter()
    a = T.imread(path) if flag is None else T.imread(path, flag)
    return a, time.perf_counter() - t0


def timed_read_device(path, flag=T.IMREAD_COLOR, wide=False):
    import torch
    T.imread_device(path, flag, wide_samples=wide)  # warm: buffers grown, kernels loaded, file in the page cache
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a = T.imread_device(path, flag, wide_samples=wide)     # returns after the status read-back, which waits for upload and kernels
    torch.cuda.synchronize()
    return a.cpu().numpy(), time.perf_counter() - t0


def both(path, nbytes, flag=None, expect=None, wide=False):
    a, dt = timed_read(path, flag)
    assert expect is None or np.array_equal(a, expect)
    text = f"{nbytes / dt / 1e6:.0f} MB/s"
    if args.device:
        b, dt = timed_read_device(path, T.IMREAD_COLOR if flag is None else flag, wide)
        assert np.array_equal(a, b)
        text += f" host, {nbytes / dt / 1e6:.0f} MB/s device"
    return text


for name, img in images.items():
    T.imwrite(d / "raw.tif", img)
    line = f"{name}: uncompressed {both(d / 'raw.tif', img.nbytes)}"
    try:
        from PIL import Image
        Image.fromarray(img[:, :, ::-1]).save(d / "lzw.tif", compression="tiff_lzw")
        line += f", LZW ({(d / 'lzw.tif').stat().st_size / 1e6:.1f} MB file) {both(d / 'lzw.tif', img.nbytes, expect=img)}"
    except ImportError:
        pass
    print(line, flush=True)
if not args.wide_only:
    f64 = rng.random((2048, 2048, 3))
    T.imwrite(d / "f64.tif", f64)
    print(f"float64 2048 x 2048 x 3 uncompressed: {both(d / 'f64.tif', f64.nbytes, T.IMREAD_UNCHANGED, expect=f64)}", flush=True)

if args.device and not args.wide_only:
    import torch
    from PIL import Image
    from camera_linearity_amd.exposure_series import ExposureSeries
    stack = d / "stack"
    stack.mkdir()
    scene = images["photo-like"].astype(np.float32)
    for k in range(7):
        frame = np.clip(scene * 2.0 ** (k - 4), 0, 255).astype(np.uint8)
        Image.fromarray(frame[:, :, ::-1]).save(stack / f"{2 ** k}ms bf 5x scene.tif", compression="tiff_lzw")
    x = np.linspace(0.0, 1.0, 256)
    icrf = np.stack([x ** 2.2] * 3, axis=1)
    icrf_diff = np.gradient(icrf, x, axis=0)

    def load_and_merge(device_decode):
        t0 = time.perf_counter()
        (series,) = ExposureSeries.from_dir_path(stack, use_cupy=True)
        series.load_value_images(device_decode=device_decode)
        t1 = time.perf_counter()
        series.process_HDR_image(icrf, icrf_diff)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return series.merged_image_set.host_arrays()[0], t1 - t0, t2 - t0

    results = {}
    for device_decode in (False, True):
        load_and_merge(device_decode)
        results[device_decode] = load_and_merge(device_decode)
        val, t_load, t_all = results[device_decode]
        print(f"7 x 4096 x 4096 x 3 LZW stack, {'device' if device_decode else 'host'} decode: load {t_load * 1e3:.0f} ms, "
              f"load + merge {t_all * 1e3:.0f} ms", flush=True)
    assert np.array_equal(results[False][0].view(np.uint64), results[True][0].view(np.uint64))       # the same bits either way


def write_u16_lzw(path, a):
    """(H, W, 3) uint16 BGR as an LZW + Predictor 2 file with imwrite's strips. LZW is byte-oriented, so the host build's encoder takes
    the differenced samples as rows of W * 6 one-byte pixels; the IFD says what they are."""
    from camera_linearity_amd import _native as nat
    lib = nat.host_lib()
    rgb = np.ascontiguousarray(a[:, :, ::-1])
    stored = rgb.copy()
    stored[:, 1:] -= rgb[:, :-1]                                        # modulo 65536, per sample
    H, W, S = a.shape
    row = W * S * 2
    rps = T._strip_rows(H, row)
    n = -(-H // rps)
    cap = int(lib.hm_tiff_encode_payload_bytes(n, rps * row, 5))
    buf = np.empty(cap, dtype=np.uint8)
    ws = np.empty(int(lib.hm_tiff_encode_workspace_bytes(n, rps * row, 5)), dtype=np.uint8)
    tables = np.empty(2 * n + 1, dtype=np.int64)
    nat.check(lib.hm_tiff_encode_strips(stored.ctypes.data, 0, 1.0, H, row, 1, rps, 5, 1, buf.ctypes.data, cap, tables.ctypes.data,
                                        tables.ctypes.data + 8 * (n + 1), ws.ctypes.data, None), "hm_tiff_encode_strips")
    offsets, counts = tables[:n + 1], tables[n + 1:]
    assert (counts > 0).all()
    total = int(offsets[n])
    head, tail = T._file_frame(H, W, S, np.dtype(np.uint16), rps, offsets, counts, total, 5, 2)
    with open(path, "wb") as f:
        f.write(head)
        f.write(memoryview(buf)[:total])
        f.write(tail)


def write_u16_big_endian(path, a):
    """(H, W, 3) uint16 BGR as an uncompressed big-endian (MM) classic TIFF, one row per strip."""
    import struct
    H, W, S = a.shape
    data = a[:, :, ::-1].astype(">u2").tobytes()
    row = W * S * 2
    offsets = [8 + r * row for r in range(H)]
    entries = [(256, 4, [W]), (257, 4, [H]), (258, 3, [16] * S), (259, 3, [1]), (262, 3, [2]), (273, 4, offsets), (277, 3, [S]),
               (278, 4, [1]), (279, 4, [row] * H), (284, 3, [1]), (339, 3, [1] * S)]
    ifd_off = 8 + len(data)
    extra_off = ifd_off + 2 + 12 * len(entries) + 4
    ifd, extra = bytearray(struct.pack(">H", len(entries))), bytearray()
    for tag, typ, vals in entries:
        payload = struct.pack(">" + {3: "H", 4: "I"}[typ] * len(vals), *vals)
        ifd += struct.pack(">HHI", tag, typ, len(vals))
        if len(payload) <= 4:
            ifd += payload.ljust(4, b"\0")
        else:
            ifd += struct.pack(">I", extra_off + len(extra))
            extra += payload + (b"\0" if len(payload) & 1 else b"")
    ifd += struct.pack(">I", 0)
    with open(path, "wb") as f:
        f.write(struct.pack(">2sHI", b"MM", 42, ifd_off) + data + bytes(ifd) + bytes(extra))


if args.device:
    import torch
    from camera_linearity_amd import engine
    U = T.IMREAD_UNCHANGED
    images16 = {"photo-like": np.clip(ramp * (4095 / 8190) + rng.normal(size=(4096, 4096, 3)) * 8, 0, 4095).astype(np.uint16),
                "noise": rng.integers(0, 4096, (4096, 4096, 3), dtype=np.uint16)}
    for name, img in images16.items():
        T.imwrite(d / "raw16.tif", img)
        write_u16_lzw(d / "lzw16.tif", img)
        print(f"uint16 (12-bit content) {name}: uncompressed {both(d / 'raw16.tif', img.nbytes, U, expect=img, wide=True)}, "
              f"LZW + Predictor 2 ({(d / 'lzw16.tif').stat().st_size / 1e6:.1f} MB file) "
              f"{both(d / 'lzw16.tif', img.nbytes, U, expect=img, wide=True)}", flush=True)
    img = images16["photo-like"]
    write_u16_big_endian(d / "mm16.tif", img)
    print(f"uint16 big-endian uncompressed: {both(d / 'mm16.tif', img.nbytes, U, expect=img, wide=True)}", flush=True)
    f32 = rng.random((4096, 4096, 3), dtype=np.float32)
    T.imwrite(d / "f32.tif", f32)
    print(f"float32 4096 x 4096 x 3 uncompressed: {both(d / 'f32.tif', f32.nbytes, U, expect=f32, wide=True)}", flush=True)
    del f32
    stack16 = d / "stack16"
    stack16.mkdir()
    scene = images16["photo-like"].astype(np.float32)
    paths = []
    for k in range(7):
        paths.append(stack16 / f"{2 ** k}ms.tif")
        write_u16_lzw(paths[-1], np.clip(scene * 2.0 ** (k - 4), 0, 4095).astype(np.uint16))
    exposures = [2.0 ** k * 1e-3 for k in range(7)]
    icrf12 = np.stack([np.linspace(0.0, 1.0, 4096) ** 2.2] * 3, axis=1)
    dev = torch.device("cuda", 0)

    def load_and_merge_u16(device_decode):
        t0 = time.perf_counter()
        if device_decode:
            frames = [T.imread_device(p, U, device=dev, wide_samples=True) for p in paths]
        else:
            frames = [torch.as_tensor(T.imread(p, U), device=dev) for p in paths]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        val = engine.merge(frames, exposures, icrf12, bit_depth=12)["val"]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return val.cpu().numpy(), t1 - t0, t2 - t0

    results = {}
    for device_decode in (False, True):
        load_and_merge_u16(device_decode)
        results[device_decode] = load_and_merge_u16(device_decode)
        val, t_load, t_all = results[device_decode]
        print(f"7 x 4096 x 4096 x 3 12-bit LZW + Predictor 2 stack, {'device' if device_decode else 'host'} decode: load {t_load * 1e3:.0f} ms, "
              f"load + engine.merge(bit_depth=12) {t_all * 1e3:.0f} ms", flush=True)
    assert np.array_equal(results[False][0].view(np.uint64), results[True][0].view(np.uint64))       # the same bits either way
import shutil  # noqa: E402
shutil.rmtree(d)
