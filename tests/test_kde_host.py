"""Kernel density estimates on the HOST build (HostMeasurand.compute_kernel_density_estimate and kde.kernel_density_estimate on a
host measurand, libhdrmerge_host.so): against the reference's own output (tests/golden/kde.npz, make_golden_kde.py), against
scipy.stats.gaussian_kde directly, and every error the reference raises. No GPU needed."""
import json

import numpy as np
import pytest
import torch
from scipy.stats import gaussian_kde

from camera_linearity_amd import kde
from camera_linearity_amd.measurand import HostMeasurand


def assert_kde_close(est, ref, rtol=1e-11):
    """|d| <= rtol |ref| + 1e-14 max |ref| elementwise."""
    est, ref = np.asarray(est), np.asarray(ref)
    assert est.shape == ref.shape and est.dtype == np.float64
    scale = np.abs(ref).max() if ref.size else 0.0
    bad = np.abs(est - ref) > rtol * np.abs(ref) + 1e-14 * scale
    assert not bad.any(), (np.flatnonzero(bad)[:5], est[bad][:5], ref[bad][:5])


def golden_cases(z):
    for k, case in enumerate(z["cases"]):
        case = json.loads(str(case))
        keys = case["channels"] or [0, 1, 2]
        ir = None if case["included_range"] is None else tuple(case["included_range"])
        yield k, case, ir, keys


def check_against_golden(z, compute):
    for k, case, ir, keys in golden_cases(z):
        res = compute(case["data_points"], ir, case["channels"], case["use_std"])
        assert list(res) == keys, case
        for c in keys:
            est, xr = res[c]
            assert isinstance(est, np.ndarray) and isinstance(xr, np.ndarray)
            assert np.array_equal(xr, z[f"xr_{k}_{c}"]), (case, c)            # np.linspace on the host: bit-identical
            assert_kde_close(est, z[f"est_{k}_{c}"])


def scipy_kde(x, w, points):
    return gaussian_kde(x, "silverman", weights=w).evaluate(points)


def test_host_matches_reference_golden(golden):
    z = golden("kde")
    m = HostMeasurand(z["val"].copy(), z["std"].copy())
    check_against_golden(z, lambda dp, ir, ch, us: m.compute_kernel_density_estimate(dp, included_range=ir, channels=ch, use_std=us))
    check_against_golden(z, lambda dp, ir, ch, us: kde.kernel_density_estimate(m, dp, included_range=ir, channels=ch, use_std=us))


@pytest.mark.parametrize("n,m,with_std,seed", [(17, 5, False, 0), (2, 3, True, 1), (1000, 256, True, 2), (31_337, 97, False, 3),
                                               (200_000, 256, True, 4)])
def test_host_matches_scipy(n, m, with_std, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 2)) * [0.3, 2.0] + [0.1, -5.0]
    s = rng.uniform(0.05, 1.0, (n, 2)) if with_std else None
    meas = HostMeasurand(x, s)
    res = meas.compute_kernel_density_estimate(m, channels=[1, 0], use_std=with_std)
    for c in (1, 0):
        pts = np.linspace(x[:, c].min(), x[:, c].max(), m)
        assert np.array_equal(res[c][1], pts)
        assert_kde_close(res[c][0], scipy_kde(x[:, c], None if s is None else 1 / s[:, c], pts), rtol=1e-10)


def test_host_all_negative_weights_work_like_scipy():
    check_all_negative_weights(host_run)


def test_host_included_range_does_not_filter():
    """Values outside included_range still contribute; the grid alone follows it."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal((500, 3))
    res = HostMeasurand(x).compute_kernel_density_estimate(33, included_range=(-0.1, 0.2), channels=[1])
    pts = np.linspace(-0.1, 0.2, 33)
    assert np.array_equal(res[1][1], pts)
    assert_kde_close(res[1][0], scipy_kde(x[:, 1], None, pts))


def host_run(x, s=None, *a, **k):
    """The measurand factory of the host tests; tests/test_gpu_kde_limits.py passes one that builds a HipMeasurand."""
    return HostMeasurand(x, s).compute_kernel_density_estimate(*a, **k)


def check_errors_match_reference(run):
    """run(values, stds or None, data_points, **kw) -> the estimate dict: every error the reference raises."""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((6, 7, 3))
    s = rng.uniform(0.1, 1.0, x.shape)
    with pytest.raises(TypeError):                                        # use_std without std: self.std[..., c]
        run(x, None, 10, use_std=True)
    one = x.copy()
    one[..., 1] = np.nan
    one[0, 0, 1] = 0.5
    with pytest.raises(ValueError):                                       # a single counted value
        run(one, None, 10)
    none = x.copy()
    none[..., 0] = np.inf
    with pytest.raises(ValueError):                                       # nothing counted: np.min of an empty array
        run(none, None, 10)
    zero = s.copy()
    zero[..., 2] = 0.0
    zero[0, 0, 2] = zero[0, 1, 2] = 1.0
    run(x, zero, 10, channels=[2], use_std=True)                          # two counted values work
    zero[0, 1, 2] = 0.0
    with pytest.raises(ValueError):                                       # std == 0 removes all but one
        run(x, zero, 10, channels=[2], use_std=True)
    nan_std = s.copy()
    nan_std[3, 3, 0] = np.nan
    with pytest.raises(ValueError):                                       # check_finite in scipy
        run(x, nan_std, 10, use_std=True)
    mixed = s.copy()
    mixed[1, 1, 0] = -0.5
    with pytest.raises(ValueError):
        run(x, mixed, 10, use_std=True)
    const = x.copy()
    const[..., 0] = 0.3
    for std in (None, s):
        with pytest.raises(np.linalg.LinAlgError):                        # deviation M: always, with or without weights
            run(const, std, 10, use_std=std is not None)
    inf_std = s.copy()
    inf_std[..., 0] = np.inf                                              # every weight 0
    with pytest.raises(ValueError):
        run(x, inf_std, 10, channels=[0], use_std=True)


def check_inf_std_counts_with_weight_zero(run):
    """An infinite std keeps its value counted (weight 0): it moves the default range but not the estimate's shape."""
    rng = np.random.default_rng(6)
    x = rng.standard_normal((400, 1))
    s = rng.uniform(0.1, 1.0, x.shape)
    x[7, 0], s[7, 0] = 25.0, np.inf
    res = run(x, s, 50, channels=[0], use_std=True)
    assert res[0][1][-1] == 25.0
    assert_kde_close(res[0][0], scipy_kde(x[:, 0], 1 / s[:, 0], res[0][1]), rtol=1e-10)


def check_all_negative_weights(run):
    rng = np.random.default_rng(9)
    x = rng.standard_normal((300, 1))
    s = -rng.uniform(0.1, 1.0, (300, 1))
    res = run(x, s, 40, channels=[0], use_std=True)
    assert_kde_close(res[0][0], scipy_kde(x[:, 0], 1 / s[:, 0], res[0][1]), rtol=1e-10)


def test_host_errors_match_reference():
    check_errors_match_reference(host_run)


def test_host_inf_std_counts_with_weight_zero():
    check_inf_std_counts_with_weight_zero(host_run)


def test_host_dn_backed_matches_float():
    rng = np.random.default_rng(8)
    dn = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
    a = HostMeasurand.from_dn(torch.from_numpy(dn)).compute_kernel_density_estimate(77)
    b = HostMeasurand(dn.astype(np.float64) / 255).compute_kernel_density_estimate(77)
    for c in range(3):
        assert np.array_equal(a[c][1], b[c][1])
        assert np.array_equal(a[c][0], b[c][0])
        assert_kde_close(a[c][0], scipy_kde((dn[..., c].astype(np.float64) / 255).ravel(), None, a[c][1]))


def test_host_zero_data_points():
    x = np.random.default_rng(1).standard_normal((10, 3))
    res = HostMeasurand(x).compute_kernel_density_estimate(0)
    assert all(res[c][0].shape == (0,) and res[c][1].shape == (0,) for c in range(3))
