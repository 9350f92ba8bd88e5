"""CPU reference of the joint identification of the 21 coefficients and a
constant world-frame wind offset (k_ident_accum_jw, k_ident_solve24,
k_ident_sens_jw): tests/ident_wind_ref.py with three more columns, numpy
float64 on the oracle, with the kernels' formulation and iteration rule
(include/kite_nmpc/kite_nmpc.h).

The model of sample k sees the wind W0[k] + w.  Columns 0..20 of the
sensitivity are those of ``ident_wind_ref`` at that total wind.  Columns
21..23 are d x^ / d w: per RK4 stage dK = J_x dX + d f / d W, with d f / d W
from ``wind_ekf_ref.dfdw``.  f is not polynomial in the wind, so that block is
a Richardson-extrapolated central difference and comes with its own error
estimate (|D(2h) - D(h)| per stage).  This module carries that estimate
through the same RK4 recursion with |J_x| (``E``, 13 x 3, an upper bound of
what the per-stage estimates do to the columns) and through the products of
the normal equations: the tests' bars for the wind rows and columns are
multiples of it.
"""
import numpy as np

from oracle import ffi
from tests import ident_ref as ref
from tests import wind_ekf_ref as wekf

IDX, NP = ref.IDX, ref.NP
NJ = NP + 3
FD_STEPS, FD_STEPS_ALT = wekf.FD_STEPS, wekf.FD_STEPS_ALT


class WindCfg:
    """kite_ident_wind_config on the host side of the reference."""

    def __init__(self, w_scale=1.0, w_prior=(0.0, 0.0, 0.0), w_box=(3.0, 3.0, 3.0), alpha_w=0.0):
        self.w_scale = float(w_scale)
        self.w_prior = np.asarray(w_prior, dtype=np.float64).reshape(3).copy()
        self.w_box = np.broadcast_to(np.asarray(w_box, dtype=np.float64), (3,)).copy()
        self.alpha_w = float(alpha_w)


def interval(kp, x, S, E, u3, w3, h, substeps, rel=ref.FD_REL, fd_steps=FD_STEPS):
    """One sample interval under the held control u3 and the held total wind
    w3: (x, S 13 x 24, E 13 x 3) -> (x+, S+, E+)."""
    x = np.array(x, dtype=np.float64); S = np.array(S, dtype=np.float64); E = np.array(E, dtype=np.float64)
    u3 = np.asarray(u3, dtype=np.float64); w3 = np.asarray(w3, dtype=np.float64).reshape(3)
    hs = h / substeps
    for _ in range(substeps):
        xs, Ss, Es = x, S, E
        ax, aS, aE = x.copy(), S.copy(), E.copy()
        for st in range(4):
            Fw, eFw = wekf.dfdw(kp, xs, u3, w3, fd_steps)       # sets and clears the oracle's wind itself
            ffi.set_wind(w3)
            try:
                k = ffi.rhs(kp, xs, u3)
                Jx = ffi.rhs_jac(kp, xs, u3)[:, :13]
                Fp = ref.dfdp(kp, xs, u3, rel)
            finally:
                ffi.set_wind(None)
            dK = Jx @ Ss + np.hstack([Fp, Fw])
            dE = np.abs(Jx) @ Es + eFw
            wa = hs / 6.0 if st in (0, 3) else hs / 3.0
            wn = 0.5 * hs if st < 2 else hs
            ax = ax + wa * k; aS = aS + wa * dK; aE = aE + wa * dE
            xs = x + wn * k; Ss = S + wn * dK; Es = E + wn * dE
        x, S, E = ax, aS, aE
    return x, S, E


def sens(kp, x13, u3, w3, h, substeps, rel=ref.FD_REL, fd_steps=FD_STEPS):
    """kite_nmpc_ident_sens_joint for one item: (x+, S 13 x 24 unscaled, E 13 x 3
    the propagated error estimate of columns 21..23)."""
    return interval(kp, x13, np.zeros((13, NJ)), np.zeros((13, 3)), u3, w3, h, substeps, rel, fd_steps)


def scales24(row, wc):
    return np.r_[ref.scales(row), [wc.w_scale] * 3]


def normal(row, p21, w, X, U, W0, cfg, wc, fd_steps=FD_STEPS, sums=False):
    """One evaluation for one kite at the parameter values p21 and the wind
    offset w: (A 24 x 24, g 24, cost, EA 24 x 24, Eg 24) in the scaled variables;
    EA and Eg bound what the finite difference's error estimate does to A and
    g (zero outside the wind rows and columns).  W0: (T, 3) or None (zeros)."""
    row = np.asarray(row, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(3)
    s = scales24(row, wc)
    z = np.r_[(np.asarray(p21, dtype=np.float64) - row[IDX]) / s[:NP], (w - wc.w_prior) / wc.w_scale]
    kp = ref.with_p(row, p21)
    T, L = U.shape[0], int(cfg.segment)
    Q = np.array(list(cfg.Q))
    A = np.zeros((NJ, NJ)); g = np.zeros(NJ); c = 0.0
    EA = np.zeros((NJ, NJ)); Eg = np.zeros(NJ)
    for k0 in range(0, T, L):
        x, S, E = X[k0].copy(), np.zeros((13, NJ)), np.zeros((13, 3))
        for k in range(k0, min(k0 + L, T)):
            wk = w if W0 is None else W0[k] + w
            x, S, E = interval(kp, x, S, E, U[k], wk, cfg.h, int(cfg.substeps), fd_steps=fd_steps)
            e = X[k + 1] - x
            St = S * s[None, :]
            Et = np.zeros((13, NJ)); Et[:, NP:] = E * wc.w_scale
            A += St.T @ (Q[:, None] * St)
            g += St.T @ (Q * e)
            c += float(e @ (Q * e))
            cross = np.abs(St).T @ (Q[:, None] * Et)
            EA += cross + cross.T
            Eg += Et.T @ (Q * np.abs(e))
    if sums:
        return A / T, g / T, c / T, EA / T, Eg / T, z
    return finish((A / T, g / T, c / T, EA / T, Eg / T, z), cfg.alpha, wc.alpha_w)


def finish(sums, alpha, alpha_w):
    """The prior terms on the data sums of ``normal(..., sums=True)``: the sums do
    not depend on alpha and alpha_w, so a test computes them once per log."""
    A, g, c, EA, Eg, z = sums
    reg = np.r_[[alpha] * NP, [alpha_w] * 3]
    return A + np.diag(reg), g - reg * z, c + float(reg @ (z * z)), EA, Eg


def bounds(cfg, wc):
    """(lo, hi) of the 24 scaled variables."""
    lo = np.r_[-np.array(list(cfg.lb_rel)), -wc.w_box / wc.w_scale]
    hi = np.r_[np.array(list(cfg.ub_rel)), wc.w_box / wc.w_scale]
    return lo, hi


def identify(row, X, U, W0, cfg, wc, fd_steps=FD_STEPS):
    """``ident_ref.identify``'s rule with 24 variables, started at the row and
    w_prior.  Returns a dict: params (52), wind (3), z (24), cost0, cost, evals,
    status (8: the wind ends on its box), costs."""
    row = np.asarray(row, dtype=np.float64)
    s = scales24(row, wc)
    pref = row[IDX]
    lo, hi = bounds(cfg, wc)
    bad = not (np.all(np.isfinite(row)) and np.all(np.isfinite(X)) and np.all(np.isfinite(U))
               and (W0 is None or np.all(np.isfinite(W0))))
    lam = cfg.lm0
    z_trial = np.zeros(NJ)
    acc = None
    costs, evals, conv = [], 0, False
    for _ in range(int(cfg.iters)):
        if bad:
            break
        A, g, c, _, _ = normal(row, pref + s[:NP] * z_trial[:NP], wc.w_prior + wc.w_scale * z_trial[NP:], X, U, W0,
                               cfg, wc, fd_steps)
        evals += 1
        accept = np.isfinite(c) and (acc is None or c <= acc["c"])
        if accept:
            acc = dict(z=z_trial.copy(), A=A, g=g, c=c)
            costs.append(c)
            lam = max(lam / 4.0, 1e-12)
        else:
            lam = min(8.0 * lam, 1e6)
        if acc is None:
            continue
        za, ga, Aa = acc["z"], acc["g"], acc["A"]
        free = ~(((za <= lo) & (ga < 0.0)) | ((za >= hi) & (ga > 0.0)))
        step = np.zeros(NJ)
        M = Aa + lam * np.trace(Aa) / NJ * np.eye(NJ)
        try:
            Lc = np.linalg.cholesky(M[np.ix_(free, free)])
            if not np.all(np.isfinite(Lc)):
                raise np.linalg.LinAlgError
            step[free] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, ga[free]))
        except np.linalg.LinAlgError:
            lam = min(8.0 * lam, 1e6)
        z_trial = np.clip(za + step, lo, hi)
        if accept and np.abs(step).max() < cfg.tol:
            conv = True
            break
    if acc is None:
        return dict(params=row.copy(), wind=wc.w_prior.copy(), z=np.zeros(NJ), cost0=np.nan, cost=np.nan,
                    evals=evals, status=1, costs=[])
    z = acc["z"]
    st = ((2 if conv else 0) | (4 if np.any((z[:NP] <= lo[:NP]) | (z[:NP] >= hi[:NP])) else 0)
          | (8 if np.any((z[NP:] <= lo[NP:]) | (z[NP:] >= hi[NP:])) else 0))
    return dict(params=ref.with_p(row, pref + s[:NP] * z[:NP]), wind=wc.w_prior + wc.w_scale * z[NP:], z=z,
                cost0=costs[0], cost=acc["c"], evals=evals, status=st, costs=costs, g=acc["g"])


def make_log(kp_true, x0, U, w3, h, substeps):
    """A noiseless log of the true model under the controls U (T, 3) and the
    constant wind w3: X (T+1, 13)."""
    T = U.shape[0]
    X = np.zeros((T + 1, 13)); X[0] = x0
    ffi.set_wind(np.asarray(w3, dtype=np.float64).reshape(3))
    try:
        for k in range(T):
            x15 = np.zeros(15); x15[:13] = X[k]
            X[k + 1] = ffi.rk4(kp_true, x15, np.r_[U[k], 0.0], h / substeps, substeps)[:13]
    finally:
        ffi.set_wind(None)
    return X


def fixture_j(kp, T, h=0.02, substeps=2, B=4):
    """Fixture J: ``ident_wind_ref.fixture_w`` with amp = 0 -- the same draws in
    the same order (truth, mean wind, gust amplitude, phase), the gust not
    applied, so the wind is the constant the model represents exactly.  Returns
    dict(truth (B, 52), w (B, 3), U, X)."""
    x0 = ffi.synthetic_states(B, offset=3000)
    truth = np.repeat(np.asarray(kp, dtype=np.float64)[None], B, axis=0)
    w = np.zeros((B, 3)); U = np.zeros((B, T, 3)); X = np.zeros((B, T + 1, 13))
    for b in range(B):
        rng = np.random.default_rng(100 + b)
        truth[b, IDX] = truth[b, IDX] * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, NP))
        w[b] = rng.uniform(-1.5, 1.5, 3)
        rng.uniform(-0.5, 0.5, 3); rng.uniform(0.0, 6.28, 3)      # fixture W's gust: drawn, not applied
        U[b] = ref.controls(T, h, 3 + b)
        X[b] = make_log(truth[b], x0[b], U[b], w[b], h, substeps)
    return dict(truth=truth, w=w, U=U, X=X)


def errors(res_params, res_wind, truth, w_true, kp):
    """(max scaled error of the 21, max wind error in m/s) of one kite."""
    e21 = np.abs((np.asarray(res_params)[IDX] - np.asarray(truth)[IDX]) / ref.scales(kp)).max()
    return e21, np.abs(np.asarray(res_wind) - np.asarray(w_true)).max()
