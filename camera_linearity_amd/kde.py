"""Weighted Gaussian kernel density estimates on either backend: the reference's NumpyMeasurand.compute_kernel_density_estimate
(modules/measurand.py:716-761; CupyMeasurand's, modules/cupy_measurand.py:88-137), i.e. scipy.stats.gaussian_kde(values,
'silverman', weights).evaluate(np.linspace(lo, hi, data_points)) per channel.

A HIP measurand computes in libhdrmerge.so (csrc/hm_kde.hip), a host measurand (backend "numpy") in libhdrmerge_host.so; there is no
SciPy behind either. DESIGN.md 4.4.2 describes the kernels and deviation M (constant data always raise LinAlgError).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np


def kernel_density_estimate(measurand, data_points: int, included_range: Optional[Tuple[float, float]] = None,
                            channels: Optional[Sequence[int]] = None, use_std: bool = False) -> Dict[int, Tuple[np.ndarray, np.ndarray]]:
    """-> {c: (estimate float64 (data_points,), x_range float64 (data_points,))}, keys in the order of `channels`
    (default range(settings.NUM_OF_CHS)), NumPy arrays on both backends.

    Counted elements of channel c: finite values and, with use_std, std != 0; each weighs 1 / std (or 1). `included_range` sets
    the grid only, every counted value contributes. Raises like the reference: ValueError for <= 1 counted value, a NaN std or
    weights of mixed sign; TypeError for use_std without std; numpy.linalg.LinAlgError for constant data."""
    from .measurand import HipMeasurand
    if not isinstance(measurand, HipMeasurand):
        raise TypeError(f"expected a Measurand, got {type(measurand)}")
    if measurand.backend not in ("hip", "numpy"):
        raise ValueError(f"unknown backend {measurand.backend!r}")
    return measurand._kernel_density_estimate(data_points, included_range, channels, use_std)
