"""Kernel density estimates on the MI355X (hm_kde.hip through kde.kernel_density_estimate): against the reference's own output
(tests/golden/kde.npz), against scipy.stats.gaussian_kde and the host build, reproducible bits (repeated calls and a graph replay of
the C-ABI launches), and 64-bit element indexing."""
import ctypes as C

import numpy as np
import pytest
import torch

from camera_linearity_amd import _native as nat
from camera_linearity_amd import engine, kde
from camera_linearity_amd.measurand import HipMeasurand, HostMeasurand

from test_kde_host import assert_kde_close, check_against_golden, scipy_kde

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def dev_kde(val, std=None, **kw):
    return kde.kernel_density_estimate(HipMeasurand(torch.as_tensor(val, device=DEV), None if std is None else torch.as_tensor(std, device=DEV)),
                                       **kw)


def test_device_matches_reference_golden(golden):
    z = golden("kde")
    m = HipMeasurand(torch.as_tensor(z["val"], device=DEV), torch.as_tensor(z["std"], device=DEV))
    calls = nat.hip_lib.calls.get("hm_kde_evaluate", 0)
    check_against_golden(z, lambda dp, ir, ch, us: kde.kernel_density_estimate(m, dp, included_range=ir, channels=ch, use_std=us))
    assert nat.hip_lib.calls["hm_kde_evaluate"] > calls
    with pytest.raises(NotImplementedError, match="kde.kernel_density_estimate"):
        m.compute_kernel_density_estimate(10)


@pytest.mark.parametrize("n,m,with_std,seed", [(2, 3, True, 1), (1000, 256, True, 2), (31_337, 97, False, 3), (200_000, 256, True, 4)])
def test_device_matches_scipy(n, m, with_std, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 2)) * [0.3, 2.0] + [0.1, -5.0]
    s = rng.uniform(0.05, 1.0, (n, 2)) if with_std else None
    res = dev_kde(x, s, data_points=m, channels=[1, 0], use_std=with_std)
    assert list(res) == [1, 0]
    for c in (1, 0):
        assert_kde_close(res[c][0], scipy_kde(x[:, c], None if s is None else 1 / s[:, c], res[c][1]), rtol=1e-10)


def test_device_matches_host_1080p_with_std():
    g = torch.Generator(device=DEV).manual_seed(3)
    val = torch.randn((1080, 1920, 3), dtype=torch.float64, device=DEV, generator=g) * 0.01
    std = torch.rand((1080, 1920, 3), dtype=torch.float64, device=DEV, generator=g) * 0.01 + 0.001
    val[5, 7, 1], std[9, 9, 2], std[10, 10, 0] = float("nan"), 0.0, float("inf")
    d = kde.kernel_density_estimate(HipMeasurand(val, std), 256, use_std=True)
    h = HostMeasurand(val.cpu().numpy(), std.cpu().numpy()).compute_kernel_density_estimate(256, use_std=True)
    for c in range(3):
        assert np.array_equal(d[c][1], h[c][1])
        assert_kde_close(d[c][0], h[c][0])


@pytest.mark.parametrize("shape,m", [((37, 1), 5), ((101, 13, 2), 1025), ((7, 11, 5), 2), ((3001, 5), 1)])
def test_device_odd_sizes_and_channel_counts(shape, m):
    rng = np.random.default_rng(shape[0])
    x = rng.standard_normal(shape) * 3.0 + 1.0
    s = rng.uniform(0.5, 2.0, shape)
    Cc = shape[-1]
    res = dev_kde(x, s, data_points=m, channels=list(range(Cc))[::-1], use_std=True)
    for c in range(Cc):
        xs, ss = x[..., c].ravel(), s[..., c].ravel()
        assert_kde_close(res[c][0], scipy_kde(xs, 1 / ss, np.linspace(xs.min(), xs.max(), m)), rtol=1e-10)


def test_device_narrow_range_skips_exactly():
    """A grid far narrower than the data: most tiles lie beyond the underflow distance of every grid point and are skipped;
    the estimate still matches scipy (whose skipped pairs are exactly 0.0)."""
    rng = np.random.default_rng(12)
    x = np.sort(rng.standard_normal((300_000, 1)) * 50.0, axis=0)          # sorted: whole tiles far from the grid
    res = dev_kde(x, data_points=64, included_range=(-0.5, 0.25), channels=[0])
    assert_kde_close(res[0][0], scipy_kde(x[:, 0], None, np.linspace(-0.5, 0.25, 64)), rtol=1e-10)
    far = dev_kde(x, data_points=8, included_range=(1e6, 2e6), channels=[0])
    assert np.array_equal(far[0][0], np.zeros(8))


def test_device_bits_repeat_and_graph_replay():
    g = torch.Generator(device=DEV).manual_seed(8)
    val = torch.randn((517, 300, 3), dtype=torch.float64, device=DEV, generator=g)
    std = torch.rand((517, 300, 3), dtype=torch.float64, device=DEV, generator=g) + 0.1
    a = engine.kernel_density_estimate(val, std, 300, None, [0, 1, 2])
    b = engine.kernel_density_estimate(val, std, 300, None, [0, 1, 2])
    for c in range(3):
        assert np.array_equal(a[c][0], b[c][0])
    n, Cc, m, c = val.numel(), 3, 300, 1
    mom_ref = torch.empty(nat.HM_KDE_MOMENTS, dtype=torch.float64, device=DEV)
    wsb = nat.hip_lib.hm_kde_workspace_bytes(n, Cc, m)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    nat.check(nat.hip_lib.hm_kde_moments(val.data_ptr(), std.data_ptr(), n, Cc, c, mom_ref.data_ptr(), ws.data_ptr(), wsb,
                                         nat.current_stream_ptr(DEV)))
    h, scale, _ = engine.kde_bandwidth(mom_ref.cpu().numpy())
    grid = torch.as_tensor(a[c][1], device=DEV)
    mom = torch.empty_like(mom_ref)
    out = torch.empty(m, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = nat.current_stream_ptr(DEV)
        nat.check(nat.hip_lib.hm_kde_moments(val.data_ptr(), std.data_ptr(), n, Cc, c, mom.data_ptr(), ws.data_ptr(), wsb, st))
        nat.check(nat.hip_lib.hm_kde_evaluate(val.data_ptr(), std.data_ptr(), n, Cc, c, h, scale, grid.data_ptr(), m, out.data_ptr(),
                                              ws.data_ptr(), wsb, st))
    for _ in range(2):
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mom, mom_ref)
        assert np.array_equal(out.cpu().numpy(), a[c][0])


def test_device_64bit_indexing():
    """n * C > 2^31 float64 elements (17 GB, C = 1), four distinct values: against the closed form sum_v count_v exp(...)."""
    vals = np.array([-0.75, 0.0, 0.5, 2.0])
    n = (1 << 31) + (1 << 20)
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < n * 8 + (2 << 30):
        pytest.fail(f"the 64-bit indexing test needs {n * 8 / 2**30:.0f} GiB of device memory, {free / 2**30:.0f} GiB free")
    x = torch.empty((n, 1), dtype=torch.float64, device=DEV)
    quads = x.view(-1, 4)
    for k, v in enumerate(vals):
        quads[:, k].fill_(float(v))
    m = 16
    res = kde.kernel_density_estimate(HipMeasurand(x), m, channels=[0])
    del x, quads
    torch.cuda.empty_cache()
    cnt = n // 4
    mean = vals.mean()
    var = cnt * ((vals - mean) ** 2).sum() / (n - 1)
    h = np.sqrt(var) * (0.75 * n) ** -0.2
    y = np.linspace(vals.min(), vals.max(), m)
    want = (cnt * np.exp(-0.5 * ((vals[:, None] - y[None, :]) / h) ** 2)).sum(0) / (n * np.sqrt(2 * np.pi) * h)
    assert np.array_equal(res[0][1], y)
    np.testing.assert_allclose(res[0][0], want, rtol=1e-8, atol=0)
