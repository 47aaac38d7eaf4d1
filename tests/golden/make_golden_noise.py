#!/usr/bin/env python3
"""Generate tests/golden/noise.npz by RUNNING the reference's noise-profile tooling (modules/video_processing.py:12-133).

Reuses make_golden.py's shims (stub `cv2`, stub `read_config`) by importing that module; like its case_welford, the
reference's `cv.VideoCapture` and `gf.video_frame_generator` are replaced in memory so that two seeded uint8 clips stand in
for two video files. Evaluated as written:
  - compute_noise_profiles([clip_a, clip_b])          -> profiles (256, 256, 3) int64 and the uint8 mean frame
  - _calculate_STD(profiles[:, :, c]) for every c     -> std (256, 3) float64, with `math` injected into the module
                                                         (deviation L: :130 calls math.sqrt without importing math)
  - clean_data_edges on a copy of every channel       -> cleaned (256, 256, 3)
  - clean_data_edges on a few extra seeded near-diagonal (256, 256) int64 arrays -> extra_in / extra_out

Usage:  python tests/golden/make_golden_noise.py        (writes tests/golden/noise.npz)
"""
import math
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import make_golden as mg  # noqa: E402  (installs the reference shims on import)


def clips():
    rng = np.random.default_rng(21)
    h, w = 24, 40
    base = rng.integers(8, 248, (h, w, 3)).astype(np.float64)
    base[0, :4] = 255.0                                 # saturated pixels: every frame clips to 255
    base[1, :4] = 0.0                                   # dark pixels: clip to 0
    out = []
    for n in (45, 19):
        clip = np.clip(np.around(base[None] + rng.standard_normal((n, h, w, 3)) * 3.0), 0, 255).astype(np.uint8)
        k = rng.integers(0, n, 12)                      # a few elements with uniform-random values far off the diagonal
        y, x, c = rng.integers(0, h, 12), rng.integers(0, w, 12), rng.integers(0, 3, 12)
        clip[k, y, x, c] = rng.integers(0, 256, 12)
        out.append(clip)
    return h, w, out


def extra_arrays():
    """Near-diagonal integer distributions with dips, zero gaps and flat spots: every branch of the cleaner's four passes."""
    rng = np.random.default_rng(22)
    m = np.arange(256)[:, None]
    f = np.arange(256)[None, :]
    arrs = []
    for sigma, scale in ((1.5, 4000), (3.0, 900), (6.0, 300)):
        lam = scale * np.exp(-0.5 * ((f - m) / sigma) ** 2)
        a = rng.poisson(lam).astype(np.int64)
        holes = rng.random(a.shape) < 0.05
        a[holes & (np.abs(f - m) < 4 * sigma)] = 0
        flat = rng.random(a.shape) < 0.05
        a[:, 1:][flat[:, 1:]] = a[:, :-1][flat[:, 1:]]
        arrs.append(a)
    return np.stack(arrs)


def main():
    import cv2
    import general_functions as gf
    import video_processing as vp
    h, w, (clip_a, clip_b) = clips()
    by_path = {"a.avi": clip_a, "b.avi": clip_b}

    class Capture:                                      # stands in for cv.VideoCapture: only the two size queries
        def __init__(self, path): pass
        def get(self, prop): return {3: w, 4: h}[prop]
    cv2.VideoCapture = Capture
    cv2.CAP_PROP_FRAME_WIDTH, cv2.CAP_PROP_FRAME_HEIGHT = 3, 4

    def frames_of(path):
        for frame in by_path[pathlib.Path(path).name]:
            yield frame
        yield None
    gf.video_frame_generator = frames_of
    vp.math = math                                      # deviation L

    with np.errstate(all="ignore"):
        profiles, mean = vp.compute_noise_profiles([pathlib.Path("a.avi"), pathlib.Path("b.avi")])
        std = np.stack([vp._calculate_STD(profiles[:, :, c]) for c in range(3)], axis=1)
    assert profiles.dtype == np.int64 and profiles.shape == (256, 256, 3)
    assert all(profiles[..., c].sum() == (len(clip_a) + len(clip_b)) * h * w for c in range(3))
    cleaned = np.stack([vp.clean_data_edges(profiles[:, :, c].copy()) for c in range(3)], axis=2)
    extra_in = extra_arrays()
    extra_out = np.stack([vp.clean_data_edges(a.copy()) for a in extra_in])
    mg.save("noise", clip_a=clip_a, clip_b=clip_b, mean=mean, profiles=profiles, std=std, cleaned=cleaned,
            extra_in=extra_in, extra_out=extra_out)


if __name__ == "__main__":
    main()
