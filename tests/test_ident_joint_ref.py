"""CPU side of the joint identification (the 21 coefficients and a constant
wind offset per kite): the reference the GPU tests compare against
(tests/ident_joint_ref.py) is itself checked here.

  * the wind columns of S after four intervals agree between the two
    finite-difference step pairs of ``wind_ekf_ref`` within the reference's own
    propagated error estimate, and that estimate is small against the columns;
    columns 0..20 do not depend on the step pair and are ``ident_wind_ref``'s
    bitwise;
  * on fixture J (``ident_joint_ref.fixture_j``: fixture W with a constant
    wind of at most 1.5 m/s per axis, h = 0.02, substeps = 2, four kites,
    (T, L) = (8, 1), (16, 4), (19, 7), coefficient box +-0.5, wind box +-3 m/s,
    lm0 = 1e-3, tol = 1e-9, Q = 1, start at the nominal row and zero wind) the
    reference recovers the 21 and the wind within 16 evaluations, converged;
  * host surface: the joint entries are exported, ``IdentWindConfig`` mirrors
    kite_ident_wind_config, ``FleetLoop`` validates ``ident_wind="joint"``.
"""
import ctypes

import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import FleetLoop, FlightRecorder
from tests import ident_joint_ref as jref
from tests import ident_ref as ref
from tests import ident_wind_ref as wref

H, SUB = 0.02, 2
CASES = [(8, 1), (16, 4), (19, 7)]
ITERS = 16


def cfg_j(**kw):
    base = dict(h=H, substeps=SUB, lb_rel=0.5, ub_rel=0.5, lm0=1e-3, tol=1e-9, Q=[1.0] * 13, iters=ITERS)
    base.update(kw)
    return ok.ident_default_config(**base)


@pytest.fixture(scope="module")
def fixtures(kp):
    return {T: jref.fixture_j(kp, T, H, SUB) for T, _ in CASES}


def test_two_fd_settings_agree_on_S_after_four_intervals(kp, fixtures):
    d = fixtures[8]
    for b in (0, 1):
        kpt = d["truth"][b]
        out = []
        for steps in (jref.FD_STEPS, jref.FD_STEPS_ALT):
            x, S, E = d["X"][b, 0].copy(), np.zeros((13, jref.NJ)), np.zeros((13, 3))
            for k in range(4):
                x, S, E = jref.interval(kpt, x, S, E, d["U"][b, k], d["w"][b], H, SUB, fd_steps=steps)
            out.append((x, S, E))
        (x0, S0, E0), (x1, S1, E1) = out
        assert x0.tobytes() == x1.tobytes() and S0[:, :21].tobytes() == S1[:, :21].tobytes()
        diff = np.abs(S0[:, 21:] - S1[:, 21:]).max()
        est = max(E0.max(), E1.max())
        big = np.abs(S0[:, 21:]).max()
        print(f"kite {b}: wind columns after 4 intervals: max {big:.3e}, two step pairs differ by {diff:.3e}, "
              f"propagated estimates {E0.max():.3e} / {E1.max():.3e}")
        # the estimate is the plain central difference's own error (the difference
        # between the pair's two steps, h^2 growth: 4 x from the first pair to the
        # second); the extrapolated columns agree far inside it
        assert big > 1e-3 and diff <= est and est <= 1e-3 * big
        assert 3.0 < E1.max() / E0.max() < 5.0
        # the 21 columns are those of the logged-wind reference at the same wind
        x, S = d["X"][b, 0].copy(), np.zeros((13, 21))
        for k in range(4):
            x, S = wref.interval(kpt, x, S, d["U"][b, k], d["w"][b], H, SUB)
        assert S.tobytes() == S0[:, :21].tobytes() and x.tobytes() == x0.tobytes()


@pytest.mark.parametrize("T,L", CASES)
def test_joint_reference_recovers_the_21_and_the_wind(kp, fixtures, T, L):
    d = fixtures[T]
    assert np.abs(d["w"]).max() <= 1.5
    cfg, wc = cfg_j(segment=L), jref.WindCfg()
    for b in range(4):
        r = jref.identify(kp, d["X"][b], d["U"][b], None, cfg, wc)
        e21, ew = jref.errors(r["params"], r["wind"], d["truth"][b], d["w"][b], kp)
        print(f"T={T} L={L} kite {b}: scaled error of the 21 {e21:.2e}, wind error {ew:.2e} m/s, "
              f"evals {r['evals']}, status {r['status']}")
        assert r["evals"] <= ITERS and r["status"] == ok.IDENT_CONVERGED
        # the log is noiseless and the model represents it exactly, so the truth is a
        # zero of the cost; the iteration stops at the first accepted step below
        # tol = 1e-9, and with cond A up to 7e6 one more such step moves the 21 by
        # no more than about ten times that (measured: 21 <= 4.0e-10, wind <= 1.3e-12 m/s,
        # 10 to 12 evaluations)
        assert e21 <= 1e-8 and ew <= 1e-8 and r["cost"] <= r["cost0"]


# ---- host surface ----------------------------------------------------------------
JOINT_ENTRIES = ["kite_nmpc_ident_sens_joint", "kite_nmpc_ident_normal_joint", "kite_nmpc_identify_joint",
                 "kite_nmpc_identify_joint_device", "kite_nmpc_ident_joint_workspace_doubles"]


def test_the_joint_entries_are_exported():
    L = ok.lib()
    for n in JOINT_ENTRIES + ["kite_ident_wind_default_config"]:
        assert hasattr(L, n), n
        assert n in nmpc._SIGNATURES
    assert L.kite_nmpc_api_version() == 7
    assert ok.IDENT_WIND_AT_BOUND == 8


def test_ident_wind_config_mirrors_the_struct():
    assert ctypes.sizeof(ok.IdentWindConfig) == 8 * 8
    c = ok.ident_wind_default_config()
    assert c.w_scale == 1.0 and list(c.w_prior) == [0.0] * 3 and list(c.w_box) == [3.0] * 3 and c.alpha_w == 0.0
    c = ok.ident_wind_default_config(w_scale=2.0, w_box=1.5, w_prior=[1.0, 2.0, 3.0], alpha_w=10.0)
    assert c.w_scale == 2.0 and list(c.w_box) == [1.5] * 3 and list(c.w_prior) == [1.0, 2.0, 3.0] and c.alpha_w == 10.0
    # the workspace needs no device; arguments the identification refuses come back negative
    n = ok.ident_joint_workspace_doubles(cfg_j(), 5, 19)
    assert n > ok.ident_workspace_doubles(cfg_j(), 5, 19)
    with pytest.raises(ok.KiteNmpcError):
        ok.ident_joint_workspace_doubles(cfg_j(substeps=0), 5, 19)


def test_fleet_loop_validates_ident_wind_joint():
    x0 = torch.zeros((2, 15), dtype=torch.float64)
    with pytest.raises(ValueError, match="adapt"):        # the joint wind is identified: it needs adapt
        FleetLoop(None, x0, 20, 0.05, recorder=FlightRecorder(2, 4), ident_wind="joint")
    with pytest.raises(ValueError):                       # and a recorder
        FleetLoop(None, x0, 20, 0.05, ident_wind="joint")
    with pytest.raises(ValueError):
        FleetLoop(None, x0, 20, 0.05, recorder=FlightRecorder(2, 4, wind=True), ident_wind="jointly")
