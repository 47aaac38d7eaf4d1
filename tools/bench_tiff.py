#!/usr/bin/env python3
"""TIFF read throughput: 4096 x 4096 x 3 uint8 images - uncompressed, and LZW as OpenCV / libtiff write it (via PIL when it is
installed) for a smooth, a photo-like (gradient + sensor noise) and a noise image; float64 uncompressed. Pixel MB/s, second read of each file.

Without arguments: the host path (tiff_io.imread) only, no GPU needed. `--device`: the device path (tiff_io.imread_device) next to it, on
the same files in the same run - timed from the open() of the file to the synchronised status read-back, so the upload of the file's
bytes is inside - and the wall time of `ExposureSeries.from_dir_path -> load_value_images -> process_HDR_image` for a stack of
7 x 4096 x 4096 x 3 LZW frames both ways (warm: the second run of each)."""
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
args = ap.parse_args()

d = pathlib.Path(tempfile.mkdtemp())
rng = np.random.default_rng(0)
ramp = np.add.outer(np.arange(4096), np.arange(4096))[:, :, None]
images = {"smooth": (ramp // 37 % 256 * np.ones(3)).astype(np.uint8),
          "photo-like": np.clip(ramp / 40 + rng.normal(size=(4096, 4096, 3)) * 2, 0, 255).astype(np.uint8),
          "noise": (rng.random((4096, 4096, 3)) * 255).astype(np.uint8)}


def timed_read(path, flag=None):
    T.imread(path) if flag is None else T.imread(path, flag)
    t0 = time.perf_counter()
    a = T.imread(path) if flag is None else T.imread(path, flag)
    return a, time.perf_counter() - t0


def timed_read_device(path, flag=T.IMREAD_COLOR):
    import torch
    T.imread_device(path, flag)                     # warm: buffers grown, kernels loaded, file in the page cache
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a = T.imread_device(path, flag)                 # returns after the status read-back, which waits for upload and kernels
    torch.cuda.synchronize()
    return a.cpu().numpy(), time.perf_counter() - t0


def both(path, nbytes, flag=None, expect=None):
    a, dt = timed_read(path, flag)
    assert expect is None or np.array_equal(a, expect)
    text = f"{nbytes / dt / 1e6:.0f} MB/s"
    if args.device:
        b, dt = timed_read_device(path, T.IMREAD_COLOR if flag is None else flag)
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
f64 = rng.random((2048, 2048, 3))
T.imwrite(d / "f64.tif", f64)
print(f"float64 2048 x 2048 x 3 uncompressed: {both(d / 'f64.tif', f64.nbytes, T.IMREAD_UNCHANGED, expect=f64)}", flush=True)

if args.device:
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
import shutil  # noqa: E402
shutil.rmtree(d)
