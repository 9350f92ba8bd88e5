"""CPU side of the identification under a logged wind: the reference the GPU
tests compare against (tests/ident_wind_ref.py) is itself checked here on
fixture W (``ident_wind_ref.fixture_w``): h = 0.02, substeps = 2, four kites
from ``ffi.synthetic_states(offset=3000)``, the 21 perturbed by +-10 %, a wind
of at most 1.5 m/s per axis with a gust of at most 0.5 m/s at 1.5 Hz, sampled
once per interval, (T, L) = (8, 1), (16, 4), (19, 7), unbounded box.

  * the wind reference recovers the truth: scaled error <= 1e-10 within 6
    evaluations, converged (measured <= 5.4e-11);
  * the windless reference on the same logs (12 evaluations) ends farther from
    the truth than the nominal row it started from, on every kite (measured 2.2
    to 200 against 0.1): what the wind in the model is for;
  * an all-zero wind log gives ``normal`` bitwise equal to ``ident_ref.normal``;
  * host surface: the four new entries are exported, the Python wrappers refuse
    a wind of the wrong shape, ``FleetLoop(ident_wind="estimate")`` needs the
    wind EKF.
"""
import math

import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import FleetLoop, FlightRecorder
from tests import ident_ref as ref
from tests import ident_wind_ref as wref

H, SUB = 0.02, 2
INF = math.inf
CASES = [(8, 1), (16, 4), (19, 7)]          # the last: three ragged chunks, a short last segment


def _cfg(**kw):
    base = dict(h=H, substeps=SUB, lb_rel=INF, ub_rel=INF)
    base.update(kw)
    return ok.ident_default_config(**base)


def _serr(rows, truth, kp):
    return np.abs((rows[:, ref.IDX] - truth[:, ref.IDX]) / ref.scales(kp)[None, :]).max(axis=1)


@pytest.fixture(scope="module")
def fixtures(kp):
    return {T: wref.fixture_w(kp, T, H, SUB) for T, _ in CASES}


@pytest.mark.parametrize("T,L", CASES)
def test_wind_reference_recovers_the_truth(kp, fixtures, T, L):
    d = fixtures[T]
    assert np.abs(d["W"]).max() <= 2.0
    cfg = _cfg(segment=L, iters=6)
    rr = [wref.identify(kp, d["X"][b], d["U"][b], d["W"][b], cfg) for b in range(4)]
    err = _serr(np.stack([r["params"] for r in rr]), d["truth"], kp)
    print(f"T={T} L={L}: scaled error {err.tolist()}, evals {[r['evals'] for r in rr]}")
    assert np.all(err <= 1e-10)
    for r in rr:
        assert r["evals"] <= 6 and r["status"] & ok.IDENT_CONVERGED and r["cost"] <= r["cost0"]


@pytest.mark.parametrize("T,L", CASES)
def test_windless_model_ends_farther_from_the_truth_than_nominal(kp, fixtures, T, L):
    d = fixtures[T]
    cfg = _cfg(segment=L, iters=12)
    rows = np.stack([ref.identify(kp, d["X"][b], d["U"][b], cfg)["params"] for b in range(4)])
    e_id = _serr(rows, d["truth"], kp)
    e_nom = _serr(np.repeat(kp[None], 4, axis=0), d["truth"], kp)
    print(f"T={T} L={L}: windless fit {e_id.tolist()}, nominal {e_nom.tolist()}")
    assert np.all(e_id > e_nom)


def test_zero_wind_log_is_the_windless_reference_bitwise(kp, fixtures):
    d = fixtures[8]
    cfg = _cfg(segment=3)
    p21 = d["truth"][1, ref.IDX]
    A0, g0, c0 = ref.normal(kp, p21, d["X"][0], d["U"][0], cfg)
    A1, g1, c1 = wref.normal(kp, p21, d["X"][0], d["U"][0], np.zeros((8, 3)), cfg)
    assert A0.tobytes() == A1.tobytes() and g0.tobytes() == g1.tobytes() and c0 == c1


# ---- host surface ----------------------------------------------------------------
WIND_ENTRIES = ["kite_nmpc_ident_sens_wind", "kite_nmpc_ident_normal_wind", "kite_nmpc_identify_wind",
                "kite_nmpc_identify_wind_device"]


def test_the_wind_entries_are_exported():
    L = ok.lib()
    for n in WIND_ENTRIES:
        assert hasattr(L, n), n
        assert n in nmpc._SIGNATURES
    assert L.kite_nmpc_api_version() == 7


def test_wrappers_refuse_a_wind_of_the_wrong_shape(kp):
    """The shape is checked before the library is called: no device needed."""
    g = object.__new__(ok.BatchNMPC)          # no context: the checks come before any call that needs one
    B, T = 3, 5
    X, U = np.zeros((B, T + 1, 13)), np.zeros((B, T, 3))
    for bad in (np.zeros((B, T + 1, 3)), np.zeros((B, T, 4)), np.zeros((B + 1, 3)), np.zeros((T, 3)), np.zeros(3)):
        with pytest.raises(ValueError):
            g.identify(X, U, kp, _cfg(), wind=bad)
        with pytest.raises(ValueError):
            g.ident_normal(X, U, np.zeros((B, 21)), kp, _cfg(), wind=bad)
    for bad in (np.zeros((B, T, 3)), np.zeros((B + 1, 3)), np.zeros(3), np.zeros((B, 4))):
        with pytest.raises(ValueError):
            g.ident_sens(X[:, 0], U[:, 0], H, 2, kp, wind=bad)
    # (B, 3) is one wind per kite, held over the log
    w = np.arange(9.0).reshape(B, 3)
    full = ok.BatchNMPC._ident_wind(w, B, T)
    assert full.shape == (B, T, 3) and full.flags["C_CONTIGUOUS"] and np.all(full == w[:, None, :])
    assert ok.BatchNMPC._ident_wind(w, B, None) .shape == (B, 3)


def test_fleet_loop_validates_ident_wind():
    x0 = torch.zeros((2, 15), dtype=torch.float64)
    with pytest.raises(ValueError, match="wind_ekf"):
        FleetLoop(None, x0, 20, 0.05, recorder=FlightRecorder(2, 4, wind=True), ident_wind="estimate")
    with pytest.raises(ValueError):
        FleetLoop(None, x0, 20, 0.05, recorder=FlightRecorder(2, 4, wind=True), ident_wind="measured")
    with pytest.raises(ValueError):                       # the wind is logged by a recorder that owns W
        FleetLoop(None, x0, 20, 0.05, recorder=FlightRecorder(2, 4), ident_wind=torch.zeros((2, 3)))
    with pytest.raises(ValueError):
        FleetLoop(None, x0, 20, 0.05, recorder=FlightRecorder(2, 4, wind=True), ident_wind=torch.zeros((3, 3)))
    rec = FlightRecorder(2, 4)
    assert rec.W is None
    with pytest.raises(ValueError):
        rec.record_wind(torch.zeros((2, 3), dtype=torch.float64))
    rec = FlightRecorder(2, 4, wind=True)
    assert tuple(rec.W.shape) == (2, 4, 3)
    w = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], dtype=torch.float64)
    rec.record_wind(w)
    rec.record_control(torch.zeros((2, 4), dtype=torch.float64))
    assert rec.nu == 1 and torch.equal(rec.W[:, 0], w) and not rec.W[:, 1:].any()
