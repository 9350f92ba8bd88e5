"""CPU reference of the identification under a logged wind (k_ident_accum_w,
k_ident_sens_w): tests/ident_ref.py with the oracle's single-kite calls under
``ffi.set_wind``, set before each sample interval and cleared after it, so that
``ffi.rhs``, ``ffi.rhs_jac`` and ``ffi.rk4`` see the air-relative velocity
v_a = v - q^-1 (x) [0, W] (x) q of that sample.  Row k of the wind log W (T, 3)
is held over sample interval k, as U[k] is.

The 21 enter only the aerodynamic forces and moments and v_a does not depend
on them, so F_p by central differences of ``ffi.rhs`` under the wind is as exact
as it is without one (tests/ident_ref.py).  The iteration rule is
``ident_ref.identify`` itself, run on this module's ``normal``.
"""
import numpy as np

from oracle import ffi
from tests import ident_ref as ref

IDX, NP = ref.IDX, ref.NP


class _wind:
    """``with _wind(w3):`` the oracle's single-kite calls see the wind w3."""

    def __init__(self, w3):
        self.w3 = np.asarray(w3, dtype=np.float64).reshape(3)

    def __enter__(self):
        ffi.set_wind(self.w3)

    def __exit__(self, *exc):
        ffi.set_wind(None)


def interval(kp, x, S, u3, w3, h, substeps, rel=ref.FD_REL):
    """One sample interval under the held control u3 and the held wind w3."""
    with _wind(w3):
        return ref.interval(kp, x, S, u3, h, substeps, rel)


def sens(kp, x13, u3, w3, h, substeps, rel=ref.FD_REL):
    """kite_nmpc_ident_sens_wind for one item: (x+, S unscaled)."""
    return interval(kp, x13, np.zeros((13, NP)), u3, w3, h, substeps, rel)


def normal(row, p21, X, U, W, cfg):
    """``ident_ref.normal`` under the wind log W (T, 3): (A, g, cost)."""
    row = np.asarray(row, dtype=np.float64)
    s = ref.scales(row)
    z = (np.asarray(p21, dtype=np.float64) - row[IDX]) / s
    kp = ref.with_p(row, p21)
    T, L = U.shape[0], int(cfg.segment)
    Q = np.array(list(cfg.Q))
    A = np.zeros((NP, NP)); g = np.zeros(NP); c = 0.0
    for k0 in range(0, T, L):
        x, S = X[k0].copy(), np.zeros((13, NP))
        for k in range(k0, min(k0 + L, T)):
            x, S = interval(kp, x, S, U[k], W[k], cfg.h, int(cfg.substeps))
            e = X[k + 1] - x
            St = S * s[None, :]
            A += St.T @ (Q[:, None] * St)
            g += St.T @ (Q * e)
            c += float(e @ (Q * e))
    A = A / T + cfg.alpha * np.eye(NP)
    g = g / T - cfg.alpha * z
    c = c / T + cfg.alpha * float(z @ z)
    return A, g, c


def identify(row, X, U, W, cfg):
    """``ident_ref.identify`` (the same iteration rule, the same dict) on the
    model that sees the wind log W (T, 3): ``ident_ref.identify`` evaluates
    through its module's ``normal``, which is this module's for the call.  A
    non-finite wind makes every cost non-finite, none is accepted, and the
    input row comes back with status 1."""
    W = np.asarray(W, dtype=np.float64)
    saved = ref.normal
    ref.normal = lambda r, p, Xk, Uk, c: normal(r, p, Xk, Uk, W, c)
    try:
        return ref.identify(row, X, U, cfg)
    finally:
        ref.normal = saved


def make_log(kp_true, x0, U, W, h, substeps):
    """A noiseless log of the true model under the controls U (T, 3) and the
    wind W (T, 3), each row held over its sample interval: X (T+1, 13)."""
    T = U.shape[0]
    X = np.zeros((T + 1, 13)); X[0] = x0
    for k in range(T):
        x15 = np.zeros(15); x15[:13] = X[k]
        with _wind(W[k]):
            X[k + 1] = ffi.rk4(kp_true, x15, np.r_[U[k], 0.0], h / substeps, substeps)[:13]
    return X


def fixture_w(kp, T, h=0.02, substeps=2, B=4):
    """Fixture W: per kite b, rng = default_rng(100 + b) draws, in this order,
    the truth (the nominal row with the 21 scaled by 1 + 0.1 U(-1, 1)), the mean
    wind w0 = U(-1.5, 1.5)^3, the gust amplitude U(-0.5, 0.5)^3 and phase
    U(0, 6.28)^3; W[k] = w0 + amp sin(2 pi 1.5 k h + ph); U = controls(T, h, 3 + b);
    X from ``make_log``.  Returns dict(truth (B, 52), W (B, T, 3), U, X)."""
    x0 = ffi.synthetic_states(B, offset=3000)
    truth = np.repeat(np.asarray(kp, dtype=np.float64)[None], B, axis=0)
    W = np.zeros((B, T, 3)); U = np.zeros((B, T, 3)); X = np.zeros((B, T + 1, 13))
    k = np.arange(T)[:, None]
    for b in range(B):
        rng = np.random.default_rng(100 + b)
        truth[b, IDX] = truth[b, IDX] * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, NP))
        w0 = rng.uniform(-1.5, 1.5, 3)
        amp = rng.uniform(-0.5, 0.5, 3)
        ph = rng.uniform(0.0, 6.28, 3)
        W[b] = w0[None] + amp[None] * np.sin(2.0 * np.pi * 1.5 * k * h + ph[None])
        U[b] = ref.controls(T, h, 3 + b)
        X[b] = make_log(truth[b], x0[b], U[b], W[b], h, substeps)
    return dict(truth=truth, W=W, U=U, X=X)
