"""CPU reference of the aerodynamic parameter identification (k_ident_accum,
k_ident_solve, k_ident_sens): numpy float64 on the oracle, with the kernels'
formulation and iteration rule (include/kite_nmpc/kite_nmpc.h).

Discrete RK4 sensitivities in variational form: per stage dK = J_x dX + F_p,
J_x = ``ffi.rhs_jac(kp, x, u)[:, :13]`` and F_p = d f / d p from central
differences of ``ffi.rhs`` in the parameter vector.  f is at most quadratic in
the 21 (CL0 and CLa enter the drag through CLt^2, everything else is linear),
so the central difference has no truncation error: it is exact up to rounding
(test_ident_ref.py measures two step sizes against each other).  Finite
differences of ``ffi.rk4`` itself are NOT the reference: Richardson-extrapolated
they reach only 4e-8.

About 10 ms per sample interval on one CPU thread: fixtures are sized for that
and computed once per module.
"""
import numpy as np

from oracle import ffi

IDENT_FIELDS = ["CL0", "CLa_total", "CD0_total", "CYb", "Cm0", "Cma", "Cnb", "Clb", "CLq", "Cmq",
                "CYr", "Cnr", "Clr", "CYp", "Clp", "Cnp", "CLde", "CYdr", "Cmde", "Cndr", "Cldr"]
# index of each identified parameter in the 52-vector (oracle.ffi.PARAM_KEYS order)
IDX = np.array([[k for _, k in ffi.PARAM_KEYS].index(f) for f in IDENT_FIELDS])
NP = 21
FD_REL = 0.2            # central-difference step, relative to the scale s_j


def scales(row):
    """s_j = |pref_j|, 1 where that is 0."""
    pref = np.asarray(row, dtype=np.float64)[IDX]
    return np.where(pref != 0.0, np.abs(pref), 1.0)


def with_p(row, p21):
    kp = np.array(row, dtype=np.float64).copy()
    kp[IDX] = p21
    return kp


def dfdp(kp, x13, u3, rel=FD_REL):
    """d f / d p (13 x 21, unscaled) at (x13, u3) by central differences of ffi.rhs."""
    s = scales(kp)
    F = np.zeros((13, NP))
    for j in range(NP):
        d = rel * s[j]
        kpp = kp.copy(); kpm = kp.copy()
        kpp[IDX[j]] += d; kpm[IDX[j]] -= d
        F[:, j] = (ffi.rhs(kpp, x13, u3) - ffi.rhs(kpm, x13, u3)) / (kpp[IDX[j]] - kpm[IDX[j]])
    return F


def interval(kp, x, S, u3, h, substeps, rel=FD_REL):
    """One sample interval: (x, S = dx/dp 13 x 21) -> (x+, S+) by `substeps` RK4
    substeps of h / substeps under the held control."""
    x = np.array(x, dtype=np.float64); S = np.array(S, dtype=np.float64)
    u3 = np.asarray(u3, dtype=np.float64)
    hs = h / substeps
    for _ in range(substeps):
        xs, Ss = x, S
        ax, aS = x.copy(), S.copy()
        for st in range(4):
            k = ffi.rhs(kp, xs, u3)
            dK = ffi.rhs_jac(kp, xs, u3)[:, :13] @ Ss + dfdp(kp, xs, u3, rel)
            wa = hs / 6.0 if st in (0, 3) else hs / 3.0
            wn = 0.5 * hs if st < 2 else hs
            ax = ax + wa * k; aS = aS + wa * dK
            xs = x + wn * k; Ss = S + wn * dK
        x, S = ax, aS
    return x, S


def sens(kp, x13, u3, h, substeps, rel=FD_REL):
    """kite_nmpc_ident_sens for one item: (x+, S unscaled)."""
    return interval(kp, x13, np.zeros((13, NP)), u3, h, substeps, rel)


def normal(row, p21, X, U, cfg):
    """One evaluation for one kite at the parameter values p21: (A, g, cost) in
    the scaled variables.  cfg: an IdentConfig (h, substeps, segment, Q, alpha)."""
    row = np.asarray(row, dtype=np.float64)
    s = scales(row)
    z = (np.asarray(p21, dtype=np.float64) - row[IDX]) / s
    kp = with_p(row, p21)
    T, L = U.shape[0], int(cfg.segment)
    Q = np.array(list(cfg.Q))
    A = np.zeros((NP, NP)); g = np.zeros(NP); c = 0.0
    for k0 in range(0, T, L):
        x, S = X[k0].copy(), np.zeros((13, NP))
        for k in range(k0, min(k0 + L, T)):
            x, S = interval(kp, x, S, U[k], cfg.h, int(cfg.substeps))
            e = X[k + 1] - x
            St = S * s[None, :]
            A += St.T @ (Q[:, None] * St)
            g += St.T @ (Q * e)
            c += float(e @ (Q * e))
    A = A / T + cfg.alpha * np.eye(NP)
    g = g / T - cfg.alpha * z
    c = c / T + cfg.alpha * float(z @ z)
    return A, g, c


def projected_gradient(z, g, lo, hi):
    """g with the components removed that push an on-bound variable outward."""
    act = ((z <= lo) & (g < 0.0)) | ((z >= hi) & (g > 0.0))
    return np.where(act, 0.0, g)


def identify(row, X, U, cfg):
    """The iteration rule for one kite.  Returns a dict: params (52), z, cost0,
    cost, evals, status, costs (the accepted costs in order)."""
    row = np.asarray(row, dtype=np.float64)
    s = scales(row)
    pref = row[IDX]
    lo = -np.array(list(cfg.lb_rel)); hi = np.array(list(cfg.ub_rel))
    bad = not (np.all(np.isfinite(row)) and np.all(np.isfinite(X)) and np.all(np.isfinite(U)))
    lam = cfg.lm0
    z_trial = np.zeros(NP)
    acc = None
    costs, evals, conv = [], 0, False
    for _ in range(int(cfg.iters)):
        if bad:
            break
        A, g, c = normal(row, pref + s * z_trial, X, U, cfg)
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
        step = np.zeros(NP)
        M = Aa + lam * np.trace(Aa) / NP * np.eye(NP)
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
        return dict(params=row.copy(), z=np.zeros(NP), cost0=np.nan, cost=np.nan, evals=evals, status=1, costs=[])
    z = acc["z"]
    st = (2 if conv else 0) | (4 if np.any((z <= lo) | (z >= hi)) else 0)
    return dict(params=with_p(row, pref + s * z), z=z, cost0=costs[0], cost=acc["c"], evals=evals, status=st,
                costs=costs)


def make_log(kp_true, x0, U, h, substeps):
    """A noiseless log: X (T+1, 13) of the true model under the controls U (T, 3)."""
    T = U.shape[0]
    X = np.zeros((T + 1, 13)); X[0] = x0
    for k in range(T):
        x15 = np.zeros(15); x15[:13] = X[k]
        X[k + 1] = ffi.rk4(kp_true, x15, np.r_[U[k], 0.0], h / substeps, substeps)[:13]
    return X


def controls(T, h, seed, rudder=True):
    """Sinusoidal thrust, elevator and rudder that fill the controller's box
    (0.1 .. 0.15 N, +-7 degrees) at 3, 7 and 5 Hz: logs of 8 samples (0.16 s)
    then excite all 21 (cond A ~ 1e6 .. 1e7; slow 1 - 2 Hz inputs of 2/3 the
    amplitude leave 5e7 .. 8e7 at T = 8, where the damped steps need more than
    six evaluations)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) * h
    ph = rng.uniform(0, 2 * np.pi, 3)
    U = np.column_stack([0.125 + 0.025 * np.sin(2 * np.pi * 3.0 * t + ph[0]),
                         0.12 * np.sin(2 * np.pi * 7.0 * t + ph[1]),
                         0.12 * np.sin(2 * np.pi * 5.0 * t + ph[2])])
    if not rudder:
        U[:, 2] = 0.0
    return U
