"""CPU side of the wind-estimating EKF (k_ekf_wind): the reference the GPU
tests compare against (tests/wind_ekf_ref.py) is itself checked here.

  * the oracle's rhs / rhs_jac under ``set_wind`` against the 50-digit wind
    fixture (tests/golden/kite_wind_golden.json) at the project's bars, 1e-13
    for f and 1e-12 for d f / d x;
  * the helper's finite-difference d f / d W against the fixture.  Measured
    here: eps_W = 1.1e-11 (largest error over the fixture's triples and both
    step pairs of the envelope runs, relative to max(1, |entry|); entries up to
    38.6); it is rounding-limited.  The bar asserted is 1e-9.  The helper's
    own error estimate, the difference between its two step pairs, is 2e-6 at
    most: it bounds the truncation of the plain differences, which the
    extrapolation removes;
  * with a zero wind estimate, a zero wind block of Wcov and zero wind rows and
    columns of P0 the filter's 13-state block is ``oracle.ffi.ekf_step``;
  * the Python surface of the feature exists.
"""
import inspect
import json
import os

import numpy as np
import pytest

import openkite_amd as ok
from oracle import ffi
from tests import wind_ekf_ref as ref


@pytest.fixture(scope="module")
def wind_golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", "kite_wind_golden.json")) as f:
        return json.load(f)


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def test_fixture_covers_the_wind_range(wind_golden):
    winds = np.array([c["wind"] for c in wind_golden["cases"]])
    assert len(winds) >= 6
    assert np.abs(winds).max() == 1.5
    assert np.any(np.all(winds == 0.0, axis=1))


def test_zero_wind_triple_is_the_wind_free_fixture(wind_golden, golden):
    c = next(c for c in wind_golden["cases"] if not np.any(c["wind"]))
    g = next(g for g in golden["rhs"] if g["x"] == c["x"] and g["u"] == c["u"])
    np.testing.assert_array_equal(c["f"], g["f"])
    np.testing.assert_array_equal(np.array(c["Jx"]), np.array(g["J"])[:, :13])


def test_oracle_wind_rhs_and_jacobian_vs_fixture(kp, wind_golden):
    for c in wind_golden["cases"]:
        ffi.set_wind(c["wind"])
        try:
            f = ffi.rhs(kp, np.array(c["x"]), np.array(c["u"]))
            J = ffi.rhs_jac(kp, np.array(c["x"]), np.array(c["u"]))[:, :13]
        finally:
            ffi.set_wind(None)
        assert _rel(f, c["f"]) < 1e-13, (c["wind"], _rel(f, c["f"]))
        assert _rel(J, c["Jx"]) < 1e-12, (c["wind"], _rel(J, c["Jx"]))


def test_finite_difference_dfdw_vs_fixture(kp, wind_golden):
    """eps_W, the error of the reference's d f / d W (module docstring)."""
    eps, est = 0.0, 0.0
    for c in wind_golden["cases"]:
        Jw, err = ref.dfdw(kp, np.array(c["x"]), np.array(c["u"]), np.array(c["wind"]))
        eps = max(eps, _rel(Jw, c["Jw"]))
        est = max(est, float(err.max()))
        # the second step pair of the envelope runs is as good
        Jw2, _ = ref.dfdw(kp, np.array(c["x"]), np.array(c["u"]), np.array(c["wind"]), ref.FD_STEPS_ALT)
        eps = max(eps, _rel(Jw2, c["Jw"]))
    print(f"eps_W = {eps:.3e}, step-pair difference {est:.3e}")
    assert eps < 1e-9
    assert est < 1e-4


@pytest.mark.parametrize("update", [False, True])
def test_degenerate_filter_is_the_13_state_ekf(kp, update):
    B = 3
    rng = np.random.default_rng(5)
    x = ffi.synthetic_states(B, offset=600)
    u = np.column_stack([rng.uniform(0.1, 0.15, B), rng.uniform(-0.1, 0.1, (B, 2))])
    W13, V, P13 = ok.ekf_default_covariances()
    G = rng.normal(size=(B, 13, 13)) * 0.01
    z = x[:, 6:13] + rng.normal(size=(B, 7)) * 0.01
    W16 = np.zeros((16, 16)); W16[:13, :13] = W13
    for b in range(B):
        P = P13 + G[b] @ G[b].T
        P16 = np.zeros((16, 16)); P16[:13, :13] = P
        x16 = np.r_[x[b], 0.0, 0.0, 0.0]
        xr, Pr, st = ref.step(kp, x16, u[b], P16, 0.02, 1, z[b] if update else None, W16, V)
        xo, Po = ffi.ekf_step(kp, x[b], u[b], 0.02, P, z[b] if update else None, W13, V)
        assert st == 0
        np.testing.assert_allclose(xr[:13], xo, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(Pr[:13, :13], Po, rtol=1e-12, atol=1e-12)
        assert np.all(xr[13:] == 0.0)
        assert np.all(Pr[13:, :] == 0.0) and np.all(Pr[:, 13:] == 0.0)


def test_python_surface_exists():
    for name in ("wind_ekf_step", "wind_ekf_step_device", "jacobian_wind", "set_wind_device"):
        assert callable(getattr(ok.BatchNMPC, name)), name
    assert callable(ok.wind_ekf_default_covariances)
    from openkite_amd import fleet
    sig = inspect.signature(fleet.FleetLoop.__init__)
    assert sig.parameters["wind_ekf"].default is False
    assert "wind_max" in sig.parameters
    for name in ("wind_ekf", "set_wind_device"):
        assert callable(getattr(fleet.GpuStepper, name)), name
    import torch
    with pytest.raises(ValueError):
        fleet.FleetLoop(None, torch.zeros((2, 15), dtype=torch.float64), 20, 0.05, ekf=True, wind_ekf=True)
    assert (ok.EKF_NAN, ok.EKF_S_NOT_PD) == (1, 2)


def test_default_covariances_are_block_diagonal():
    W13, V13, P13 = ok.ekf_default_covariances()
    W, V, P0 = ok.wind_ekf_default_covariances()
    np.testing.assert_array_equal(W[:13, :13], W13)
    np.testing.assert_array_equal(P0[:13, :13], P13)
    np.testing.assert_array_equal(V, V13)
    np.testing.assert_array_equal(np.diag(W)[13:], [1e-4] * 3)
    np.testing.assert_array_equal(np.diag(P0)[13:], [25.0] * 3)
    assert np.count_nonzero(W - np.diag(np.diag(W))) == 0 and np.count_nonzero(P0 - np.diag(np.diag(P0))) == 0
