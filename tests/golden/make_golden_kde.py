#!/usr/bin/env python3
"""Generate tests/golden/kde.npz by RUNNING the reference's NumpyMeasurand.compute_kernel_density_estimate
(modules/measurand.py:716-761, scipy.stats.gaussian_kde(values, 'silverman', weights)) on seeded 40 x 50 x 3 arrays.

Reuses make_golden.py's shims (stub `cv2`, stub `read_config`) by importing that module. Two inputs: `val` (difference-image-like
normal values with a few NaN / +-inf values) and `std` (positive, with a few zeros, a few infs). Cases (`cases`: one JSON object
per case with data_points, included_range, channels, use_std; outputs `est_<case>_<c>` and `xr_<case>_<c>`):
  default arguments; use_std=True; included_range narrower and wider than the data, with and without std; channels=[2, 0];
  data_points 1, 2 and 513.

Usage:  python tests/golden/make_golden_kde.py        (writes tests/golden/kde.npz)
"""
import json
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import make_golden as mg  # noqa: E402  (installs the reference shims on import)

CASES = [
    dict(data_points=200, included_range=None, channels=None, use_std=False),
    dict(data_points=200, included_range=None, channels=None, use_std=True),
    dict(data_points=150, included_range=[-0.02, 0.01], channels=None, use_std=False),
    dict(data_points=150, included_range=[-0.5, 0.7], channels=None, use_std=True),
    dict(data_points=100, included_range=[-0.03, -0.029], channels=None, use_std=True),
    dict(data_points=64, included_range=None, channels=[2, 0], use_std=True),
    dict(data_points=1, included_range=None, channels=None, use_std=False),
    dict(data_points=2, included_range=None, channels=None, use_std=True),
    dict(data_points=513, included_range=None, channels=None, use_std=True),
]


def inputs():
    rng = np.random.default_rng(31)
    shape = (40, 50, 3)
    val = rng.standard_normal(shape) * np.array([0.01, 0.02, 0.015]) + np.array([0.0, 0.003, -0.002])
    std = rng.uniform(0.002, 0.02, shape)
    for bad in (np.nan, np.inf, -np.inf):
        idx = tuple(rng.integers(0, s, 5) for s in shape)
        val[idx] = bad
    std[tuple(rng.integers(0, s, 20) for s in shape)] = 0.0
    std[tuple(rng.integers(0, s, 20) for s in shape)] = np.inf
    return val, std


def main():
    val, std = inputs()
    m = mg.ref_measurand.NumpyMeasurand(val.copy(), std.copy())
    out, names = {}, []
    for k, case in enumerate(CASES):
        ir = None if case["included_range"] is None else tuple(case["included_range"])
        res = m.compute_kernel_density_estimate(case["data_points"], included_range=ir, channels=case["channels"], use_std=case["use_std"])
        keys = list(res)
        assert keys == (case["channels"] or [0, 1, 2])
        for c in keys:
            out[f"est_{k}_{c}"], out[f"xr_{k}_{c}"] = res[c]
        names.append(json.dumps(case))
    mg.save("kde", val=val, std=std, cases=np.array(names), **out)


if __name__ == "__main__":
    main()
