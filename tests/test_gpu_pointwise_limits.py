"""The operator, selection and per-frame kernels (csrc/hm_ops.hip, csrc/hm_pointwise.hip, csrc/hm_linearize.hip) on the MI355X at the
limits of their ABI: the checks of tests/test_pointwise_limits_host.py - the references, the derived bounds and every case live there - on
device buffers. Every test asserts that the device symbol ran and the host one did not.

This module alone also runs the sizes at which a lane or a wave of a grid-stride loop takes its SECOND step (only the device build has such
loops), from the CU count cu the library reports: one launch per case, inputs from one seeded generator, compared as in the host module's
families A / B / C / E.
    k_thresholds, C = 2, 3, 4 (two elements per lane, 8 workgroups of 256 per CU)            n = 2 (8 256 cu) + 10 C + 1
    k_thresholds_wide, C = 5, 7; k_unary; k_take; k_binary on (n / 3, 3) x (3,);
    k_difference_bcast, k_interpolate_bcast (one element per lane)                            n = 8 256 cu + 777
    k_binary_burst MUL, k_difference_burst, k_interpolate_burst (both stds),
    k_pow_scalar_burst SQRT and INT -3 with std (waves over 512-element chunks, 16 x 4 per CU) n = (64 cu + 5) 512 + 77
    k_weight_f64_burst, w only (balanced wave grid, 12 x 4 per CU)                            n = (48 cu + 5) 512 + 77"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from camera_linearity_amd import _native as nat
from oracle import hdr_oracle as orc

import test_pointwise_limits_host as pl
from test_pointwise_limits_host import report_observed_maxima  # noqa: F401  (prints the observed maxima after this module too)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BCAST = {"binary": "hm_binary_op", "difference": "hm_compute_difference_bcast", "interpolate": "hm_interpolate_bcast"}
LIN = {"u8": "hm_linearize_u8", "f64": "hm_linearize_f64"}


@contextlib.contextmanager
def on_device(*symbols):
    """Every one of `symbols` is called in the HIP library inside the block, none of them in the host library."""
    hip, host = nat.hip_lib.calls, nat.host_lib().calls
    before = {s: (hip[s], host[s]) for s in symbols}
    yield
    for s, (d, h) in before.items():
        assert hip[s] > d and host[s] == h, (s, hip[s] - d, host[s] - h)


@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_binary_dense(op):
    with on_device("hm_binary_op"):
        pl.check_binary_dense(DEV, op)


def test_difference():
    with on_device("hm_compute_difference"):
        pl.check_difference(DEV)


def test_interpolate():
    with on_device("hm_interpolate"):
        pl.check_interpolate(DEV)


def test_unary():
    with on_device("hm_unary_op"):
        pl.check_unary(DEV)


def test_log10_constant():
    with on_device("hm_unary_op"):
        pl.check_log10_constant(DEV)


@pytest.mark.parametrize("p", pl.EXPONENTS)
def test_pow_benign(p):
    with on_device("hm_pow_scalar"):
        pl.check_pow_benign(DEV, p)


@pytest.mark.parametrize("p_index,p", list(enumerate(pl.EXPONENTS + pl.ODD_EXPONENTS)))
def test_pow_specials(p_index, p):
    with on_device("hm_pow_scalar"):
        pl.check_pow_specials(DEV, p_index, p)


@pytest.mark.parametrize("p", [2.0, 0.5, -3.0, 2.5])
def test_pow_tail_specials(p):
    with on_device("hm_pow_scalar"):
        pl.check_pow_tail_specials(DEV, p)


def test_pow_half_at_numpy():
    with on_device("hm_pow_scalar"):
        pl.check_pow_half_at_numpy(DEV)


def test_binary_pow():
    with on_device("hm_binary_op"):
        pl.check_binary_pow(DEV)


def test_weight_f64():
    with on_device("hm_gaussian_weight_f64"):
        pl.check_weight_f64(DEV)


def test_weight_u8():
    with on_device("hm_gaussian_weight_u8"):
        pl.check_weight_u8(DEV)


def test_u8_to_unit():
    with on_device("hm_u8_to_unit_f64"):
        pl.check_u8_to_unit(DEV)


def test_take():
    with on_device("hm_take_axis"):
        pl.check_take(DEV)


@pytest.mark.parametrize("op", [0, 1, 2, 3, 4])
def test_bcast_binary(op):
    with on_device("hm_binary_op"):
        pl.check_bcast(DEV, "binary", op)


@pytest.mark.parametrize("entry", ["difference", "interpolate"])
def test_bcast_pointwise(entry):
    with on_device(BCAST[entry]):
        pl.check_bcast(DEV, entry)


def test_bad_geometry():
    """HM_EINVAL from every entry, and the same statuses as the host build case by case."""
    with on_device(*BCAST.values()):
        pl.check_bad_geometry(DEV)
    assert pl.bad_geometry_statuses(DEV) == pl.bad_geometry_statuses("cpu")


@pytest.mark.parametrize("C_", pl.THRESHOLD_CHANNELS)
def test_thresholds(C_):
    with on_device("hm_apply_thresholds"):
        pl.check_thresholds(DEV, C_)


def test_thresholds_too_wide():
    with on_device("hm_apply_thresholds"):
        pl.check_thresholds_too_wide(DEV)


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_linearize(kind):
    with on_device(LIN[kind]):
        pl.check_linearize(DEV, kind)


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_linearize_channels(kind):
    with on_device(LIN[kind]):
        pl.check_linearize_channels(DEV, kind)


def test_linearize_undefined():
    with on_device("hm_linearize_f64"):
        pl.check_linearize_undefined(DEV)


@pytest.mark.parametrize("bits", [9, 12, 16])
def test_linearize_u16(bits):
    with on_device("hm_linearize_u16"):
        pl.check_linearize_u16(DEV, bits)


# ------------------------------------------------------------------------------------------------ the second step of every grid-stride loop
ONE = [None]                                                                # one launch: all streams aligned


def cu_count():
    n, cu, lds = C.c_int(0), C.c_int(0), C.c_int(0)
    arch = C.create_string_buffer(32)
    assert nat.hip_lib.hm_device_info(C.byref(n), C.byref(cu), C.byref(lds), arch, 32) == nat.HM_OK and n.value >= 1 and cu.value >= 1
    return cu.value


def n_lane():
    return 8 * 256 * cu_count() + 777


def n_burst(blocks_per_cu=16):
    return (blocks_per_cu * 4 * cu_count() + 5) * 512 + 77


def last_rows(C_):
    """(rows, 3) x (3,) with rows * 3 >= n_lane()."""
    rows = -(-n_lane() // C_)
    return ("second step, trailing broadcast", (rows, C_), (C_, 1), (0, 1))


@pytest.mark.parametrize("C_", [2, 3, 4, 5, 7])
def test_second_step_thresholds(C_):
    n = 2 * (8 * 256 * cu_count()) + 2 * C_ * 5 + 1 if C_ <= 4 else n_lane()
    with on_device("hm_apply_thresholds"):
        pl.check_thresholds(DEV, C_, sizes=[n])


def test_second_step_unary():
    n = n_lane()
    rng = np.random.default_rng(11)
    x, s = pl.values(rng, n), pl.stds(rng, n)
    with on_device("hm_unary_op"):
        got = pl.run_unary(DEV, 0, n, x, s, configs=ONE)
    pl.assert_bits(got["out"], np.negative(x), "neg, second step")
    pl.assert_bits(got["out_std"], s, "neg std, second step")


def test_second_step_take():
    n = n_lane()
    rng = np.random.default_rng(12)
    x, s = rng.random((1, 2, n)), rng.random((1, 2, n))
    with on_device("hm_take_axis"):
        got = pl.run_take(DEV, (1, 2, n), [1], x, s, configs=ONE)
    pl.assert_bits(got["out"], x[0, 1], "take, second step")
    pl.assert_bits(got["out_std"], s[0, 1], "take std, second step")


@pytest.mark.parametrize("entry,op", [("binary", 2), ("difference", None), ("interpolate", None)])
def test_second_step_bcast(entry, op):
    with on_device(BCAST[entry]):
        pl.check_bcast(DEV, entry, op, cases=[last_rows(3)])


def test_second_step_binary_burst():
    n = n_burst()
    x1, s1, x2, s2 = pl.dense_inputs(n, 13)
    with on_device("hm_binary_op"):
        got = pl.run_binary_dense(DEV, 2, n, True, True, x1, s1, x2, s2, configs=ONE)
    with np.errstate(all="ignore"):
        rv, rs = orc.op_mul(x1, s1, x2, s2)
    pl.assert_bits(got["out"], rv, "mul, second step")
    pl.assert_bits(got["out_std"], rs, "mul std, second step")


def test_second_step_difference_burst():
    n = n_burst()
    x, sx, y, sy = pl.dense_inputs(n, 14)
    with on_device("hm_compute_difference"):
        got = pl.run_difference(DEV, n, True, True, x, sx, y, sy, configs=ONE)
    pl.assert_difference(got, x, sx, y, sy, "difference, second step")


def test_second_step_interpolate_burst():
    n = n_burst()
    x0, s0, x1, s1 = pl.dense_inputs(n, 15)
    with on_device("hm_interpolate"):
        got = pl.run_interpolate(DEV, n, True, True, x0, s0, x1, s1, configs=ONE)
    pl.assert_interpolate(got, x0, s0, x1, s1, "interpolate, second step")


@pytest.mark.parametrize("p", [0.5, -3.0])
def test_second_step_pow_burst(p):
    n = n_burst()
    rng = np.random.default_rng(16)
    x, s = 0.05 + rng.random(n), 0.01 + 0.05 * rng.random(n)
    with on_device("hm_pow_scalar"):
        got = pl.run_pow(DEV, p, n, x, s, configs=ONE)
    pl.assert_pow_benign(DEV, p, x, s, got["out"], got["out_std"], f"pow_scalar p={p}, second step")


def test_second_step_weight_burst():
    n = n_burst(12)
    v = -1.5 + 4.0 * np.random.default_rng(17).random(n)
    with on_device("hm_gaussian_weight_f64"):
        got = pl.run_weight_f64(DEV, n, v, True, False, configs=ONE)
    rw, _ = pl.weight_reference(v)
    pl.assert_close(pl.family(DEV, "gaussian weight") + " w", got["w"], rw, 1e-13, "weight w alone, second step", atol=1e-300)
