"""CPU reference of the wind-estimating EKF (k_ekf_wind): a numpy float64
filter with the kernel's semantics, built on the oracle.

f, the RK4 step and the 13 x 13 Jacobian block come from the oracle under
``oracle.ffi.set_wind`` (thread-local wind).  The oracle has no d f / d W, so
that block is a Richardson-extrapolated central difference of the oracle's
``rhs`` over the wind, with two step sizes; the same helper returns the
difference between the two plain central differences as the reference's own
error estimate.  ``fd_steps`` selects the step pair, so a
test can run the whole filter with two pairs and take the spread as the
envelope of what the finite difference does to the wind rows and columns.

As the kernel, the filter makes P symmetric after every update.  Without
that the recursion is unstable: S is factored from its lower triangle, the
update does not damp an antisymmetric part of P, and rounding noise grows by
1.4 to 1.6 per period (measured here: |P - P'| 2.7e-15 after 4 periods of the
open-loop run of test_wind_ekf.py, 2.1e-10 after 40), so that two
implementations of the same arithmetic part ways within a second of flight.
"""
import numpy as np

from oracle import ffi

FD_STEPS = (2e-3, 1e-3)          # m/s
FD_STEPS_ALT = (4e-3, 2e-3)      # the second pair of the envelope runs


def _central(kp, x13, u3, w3, h):
    J = np.zeros((13, 3))
    for k in range(3):
        wp = np.array(w3, dtype=np.float64); wm = wp.copy()
        wp[k] += h; wm[k] -= h
        ffi.set_wind(wp); fp = ffi.rhs(kp, x13, u3)
        ffi.set_wind(wm); fm = ffi.rhs(kp, x13, u3)
        J[:, k] = (fp - fm) / (wp[k] - wm[k])
    return J


def dfdw(kp, x13, u3, w3, fd_steps=FD_STEPS):
    """(d f / d W (13 x 3), error estimate (13 x 3)) at wind w3: Richardson
    extrapolation (4 D(h) - D(2h)) / 3 of central differences with the steps
    fd_steps = (2h, h); the estimate is |D(2h) - D(h)|, the difference between
    the two step pairs (three times the correction the extrapolation applies)."""
    h2, h1 = fd_steps
    try:
        D2 = _central(kp, x13, u3, w3, h2)
        D1 = _central(kp, x13, u3, w3, h1)
    finally:
        ffi.set_wind(None)
    r = (h2 / h1) ** 2
    J = (r * D1 - D2) / (r - 1.0)
    return J, np.abs(D2 - D1)


def jac16(kp, x13, u3, w3, fd_steps=FD_STEPS):
    """[d f / d x | d f / d W] (13 x 16) under wind w3."""
    ffi.set_wind(w3)
    try:
        Jx = ffi.rhs_jac(kp, x13, u3)[:, :13]
    finally:
        ffi.set_wind(None)
    Jw, _ = dfdw(kp, x13, u3, w3, fd_steps)
    return np.hstack([Jx, Jw])


def step(kp, x16, u3, P, dt, substeps=1, z7=None, W=None, V=None, fd_steps=FD_STEPS):
    """One call of the filter for one kite: returns (x16, P, status)."""
    x = np.array(x16, dtype=np.float64).copy()
    P = np.array(P, dtype=np.float64).reshape(16, 16).copy()
    u3 = np.asarray(u3, dtype=np.float64)
    h = dt / substeps
    for _ in range(substeps):
        J = np.zeros((16, 16))
        J[:13] = jac16(kp, x[:13], u3, x[13:], fd_steps)
        A = np.eye(16) + J * h
        x15 = np.zeros(15); x15[:13] = x[:13]
        ffi.set_wind(x[13:])
        try:
            x[:13] = ffi.rk4(kp, x15, np.r_[u3, 0.0], h, 1)[:13]
        finally:
            ffi.set_wind(None)
        P = A @ P @ A.T + W
    status = 0
    if z7 is not None:
        S = P[6:13, 6:13] + V
        try:
            L = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            return x, P, 2
        Si = lambda r: np.linalg.solve(L.T, np.linalg.solve(L, r))
        x = x + P[:, 6:13] @ Si(np.asarray(z7, dtype=np.float64) - x[6:13])
        P = P - P[:, 6:13] @ Si(P[6:13, :])
        P = 0.5 * (P + P.T)
    return x, P, status


def step_batch(kp, x16, u3, P, dt, substeps=1, z7=None, W=None, V=None, fd_steps=FD_STEPS):
    B = x16.shape[0]
    xo = np.zeros((B, 16)); Po = np.zeros((B, 16, 16)); st = np.zeros(B, dtype=np.int32)
    for b in range(B):
        xo[b], Po[b], st[b] = step(kp, x16[b], u3[b], P[b], dt, substeps, None if z7 is None else z7[b], W, V,
                                   fd_steps)
    return xo, Po, st
