"""Shared cases of the per-kite estimator tests (test_ekf_perkite_ref.py on the
CPU, test_ekf_perkite.py on the GPU): the heterogeneous rows, the filter inputs
and each kite's reference under its own row.

The references take the parameter row per call, so kite b's reference is a
batch of one under rows[b] (as perkite_cases.oracle_step): ``ffi.ekf_step`` for
k_ekf, ``wind_ekf_ref.step`` for the wind filter.  Rows: perkite_cases.rows_for.
Inputs: test_wind_ekf._inputs (states at offset 800, DT = 0.02, a wind block of
0.04 in P); k_ekf takes their 13-state part.  Everything is computed once per
case and shared: treat what these functions return as read-only."""
import functools

import numpy as np

import openkite_amd as ok
from oracle import ffi
from tests import perkite_cases as pc
from tests import wind_ekf_ref as ref

BMAX = 130                    # 32 full blocks of four kites and a ragged one
DT = 0.02
PWW = 0.04                    # wind block of the test covariance (test_wind_ekf.py)
GAP = pc.GAP                  # a reference under the wrong row is this many parity bars away
# parity bars of test_ekf.py / test_wind_ekf.py
X_RTOL, P_RTOL, ATOL = 1e-12, 1e-11, 1e-13
WIND_FLOOR = 1e-11


def rows_for(B, seed=pc.SEED):
    return pc.rows_for(B, seed)


def nominal_rows(B):
    return np.repeat(ffi.load_params()[None], B, axis=0)


@functools.lru_cache(maxsize=None)
def wind_inputs(B=BMAX):
    """test_wind_ekf._inputs(B): (x16, u, P, z, W, V)."""
    from tests.test_wind_ekf import _inputs
    return _inputs(B)


def ekf_inputs(B=BMAX):
    """The 13-state part of wind_inputs: (x13, u, P, z, W, V)."""
    x16, u, P, z, W, V = wind_inputs(B)
    return (x16[:, :13].copy(), u, np.ascontiguousarray(P[:, :13, :13]), z, np.ascontiguousarray(W[:13, :13]), V)


def _row(rows, b):
    return rows if rows.ndim == 1 else rows[b]


def ekf_ref(rows, x, u, P, dt, substeps, z, W, V):
    """k_ekf's reference kite by kite: `substeps` calls of ffi.ekf_step over
    dt / substeps, the update on the last (as FleetLoop drives the filter)."""
    B = x.shape[0]
    xo, Po = x.copy(), P.copy()
    for b in range(B):
        for s in range(substeps):
            zz = z[b] if (z is not None and s == substeps - 1) else None
            xo[b], Po[b] = ffi.ekf_step(_row(rows, b), xo[b], u[b], dt / substeps, Po[b], zz, W, V)
    return xo, Po


def wind_ref(rows, x16, u, P, dt, substeps, z, W, V, fd_steps=ref.FD_STEPS):
    """The wind filter's reference kite by kite under rows[b] (or one row)."""
    B = x16.shape[0]
    xo = np.zeros((B, 16)); Po = np.zeros((B, 16, 16)); st = np.zeros(B, dtype=np.int32)
    for b in range(B):
        xo[b], Po[b], st[b] = ref.step(_row(rows, b), x16[b], u[b], P[b], dt, substeps,
                                       None if z is None else z[b], W, V, fd_steps)
    return xo, Po, st


@functools.lru_cache(maxsize=None)
def ekf_reference(B, substeps, update, own_rows=True):
    """k_ekf's reference on the first B kites of the inputs under rows_for(B)
    (own_rows) or the nominal row."""
    x, u, P, z, W, V = (a[:B] if i < 4 else a for i, a in enumerate(ekf_inputs()))
    rows = rows_for(B) if own_rows else ffi.load_params()
    return ekf_ref(rows, x, u, P, DT, substeps, z if update else None, W, V)


@functools.lru_cache(maxsize=None)
def wind_reference(B, substeps, update, own_rows=True, alt=False):
    """The wind filter's reference on the first B kites of the inputs; alt: the
    second finite-difference step pair (the envelope run)."""
    x16, u, P, z, W, V = (a[:B] if i < 4 else a for i, a in enumerate(wind_inputs()))
    rows = rows_for(B) if own_rows else ffi.load_params()
    return wind_ref(rows, x16, u, P, DT, substeps, z if update else None, W, V,
                    ref.FD_STEPS_ALT if alt else ref.FD_STEPS)


# ---- the measures of the bars ------------------------------------------------------
def worst(got, want, rtol, atol=ATOL):
    """Largest error in units of the assert_allclose bar atol + rtol |want|."""
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


def worst_per_kite(got, want, rtol, atol=ATOL):
    e = np.abs(got - want) / (atol + rtol * np.abs(want))
    return e.reshape(e.shape[0], -1).max(1)


def wind_entries(x, P):
    return np.concatenate([x[..., 13:].reshape(-1), P[..., 13:, :].reshape(-1), P[..., :13, 13:].reshape(-1)])


def wind_bar(a, b):
    """(envelope, bar) of the wind rows and columns from the reference's two
    runs a, b: 10 x the envelope, not below 1e-11 (test_wind_ekf._wind_bar)."""
    env = float(np.abs(wind_entries(a[0], a[1]) - wind_entries(b[0], b[1])).max())
    return env, max(10.0 * env, WIND_FLOOR)


# ---- the open-loop run -----------------------------------------------------------
OL_B, OL_T, OL_DT, OL_SEED = 8, 40, 0.02, 42     # test_wind_ekf.open_loop's


@functools.lru_cache(maxsize=None)
def open_loop_truth():
    """test_wind_ekf.open_loop's truth (8 kites, 40 periods of 0.02 s, winds of
    0.3 .. 0.8 m/s, seed 42, states at offset 900, a fixed control), with one
    change: every kite is integrated under its own row of rows_for(8).
    Returns dict(rows, wind, mag, u, x0, z (T, B, 7))."""
    B, T, dt = OL_B, OL_T, OL_DT
    rows = rows_for(B)
    rng = np.random.default_rng(OL_SEED)
    xt = ffi.synthetic_states(B, offset=900)
    x0 = xt.copy()
    mag = rng.uniform(0.3, 0.8, B)
    d = rng.normal(size=(B, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    wind = d * mag[:, None]
    u = np.tile([0.125, 0.0, 0.0], (B, 1))
    z = np.zeros((T, B, 7))
    for t in range(T):
        for b in range(B):
            x15 = np.zeros(15); x15[:13] = xt[b]
            ffi.set_wind(wind[b])
            try:
                xt[b] = ffi.rk4(rows[b], x15, np.r_[u[b], 0.0], dt, 1)[:13]
            finally:
                ffi.set_wind(None)
        z[t] = xt[:, 6:13]
    return dict(rows=rows, wind=wind, mag=mag, u=u, x0=x0, z=z)


def open_loop_start():
    """(x16, P) every filter of the open-loop run starts from: W = 0, P0."""
    tr = open_loop_truth()
    _, _, P0 = ok.wind_ekf_default_covariances()
    xe = np.zeros((OL_B, 16)); xe[:, :13] = tr["x0"]
    return xe, np.repeat(P0[None], OL_B, axis=0)


@functools.lru_cache(maxsize=None)
def open_loop_reference(own_rows=True, alt=False):
    """The reference filter over the open-loop run, with each kite's own row
    (own_rows) or the nominal row in the filter: (x16, P) after the T periods."""
    tr = open_loop_truth()
    rows = tr["rows"] if own_rows else ffi.load_params()
    W, V, _ = ok.wind_ekf_default_covariances()
    xe, P = open_loop_start()
    for t in range(OL_T):
        xe, P, st = wind_ref(rows, xe, tr["u"], P, OL_DT, 1, tr["z"][t], W, V,
                             ref.FD_STEPS_ALT if alt else ref.FD_STEPS)
        assert not st.any()
    return xe, P


def wind_error_ratio(x16):
    """Final / initial wind error per kite (the initial estimate is W = 0)."""
    tr = open_loop_truth()
    return np.linalg.norm(x16[:, 13:] - tr["wind"], axis=1) / tr["mag"]
