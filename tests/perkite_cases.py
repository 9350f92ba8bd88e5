"""Shared cases of the per-kite controller model tests (test_params_abi.py on
the CPU, test_perkite_model.py on the GPU): the heterogeneous rows, the states,
and each kite's oracle reference under its own row.

The oracle takes the parameter row per call, so kite b's reference is a batch
of one under rows[b]; nothing in the oracle knows about a batch of models."""
import functools

import numpy as np

import openkite_amd as ok
from oracle import ffi

M, K = 2, 16
B9 = 9              # crosses the homogeneous sensitivity kernel's 8-kite block
SEED = 3            # chosen on the CPU: test_params_abi.test_oracle_is_sensitive_to_the_rows_*
GAP = 1e3           # an oracle under the wrong row is this many parity bars away


def rows_for(B, seed=SEED):
    """+-10 % over the 21 identified fields, plus mass on kite 1 and Ixx on kite
    2 (where the batch has them): inv_mass and the J^-1 entries differ too."""
    kp = ffi.load_params()
    rows = ok.perturb_params(kp, B, 0.10, seed, fields=ok.IDENT_FIELDS)
    f = ok.nmpc._PARAM_FIELDS
    if B > 1:
        rows[1, f.index("mass")] *= 1.08
    if B > 2:
        rows[2, f.index("Ixx")] *= 0.93
    return rows


def states(B, offset, Nh=20):
    cv = ffi.cfg_vector(ffi.node_config(N=Nh))
    xs = ffi.synthetic_states(B, offset=offset)
    x0 = np.zeros((B, 15))
    x0[:, :13] = xs
    for b in range(B):
        x0[b, 13] = ffi.closest_point(cv, xs[b, 6:9])
    return x0


def oracle_step(rows, cv, Nh, x, X, U, warm, wind=None):
    """One RTI step of every kite under its own row (rows (B, 52), or one row
    for all); X, U updated in place as ffi.rti_step does."""
    B = x.shape[0]
    u0 = np.zeros((B, 4)); diag = np.zeros((B, 6)); st = np.zeros(B, dtype=np.int32)
    for b in range(B):
        Xb = X[b:b + 1].copy(); Ub = U[b:b + 1].copy()
        r = rows if rows.ndim == 1 else rows[b]
        u, d, s = ffi.rti_step(r, cv, Nh, M, K, x[b:b + 1], Xb, Ub, warm=warm,
                               wind=None if wind is None else wind[b:b + 1])
        X[b] = Xb[0]; U[b] = Ub[0]; u0[b] = u[0]; diag[b] = d[0]; st[b] = s[0]
    return u0, diag, st


@functools.lru_cache(maxsize=None)
def oracle_loop(Nh, B, steps, offset, own_rows=True, seed=SEED):
    """Closed oracle loop (the next measured state is the plan's node 1) under
    the per-kite rows (own_rows) or the nominal row: per step
    (x, u0, X, U, diag, status), computed once and shared (treat as read-only)."""
    cv = ffi.cfg_vector(ffi.node_config(N=Nh))
    rows = rows_for(B, seed) if own_rows else ffi.load_params()
    x = states(B, offset, Nh)
    X = np.zeros((B, Nh + 1, 15)); U = np.zeros((B, Nh, 4))
    out = []
    for step in range(steps):
        u0, diag, st = oracle_step(rows, cv, Nh, x, X, U, warm=int(step > 0))
        out.append((x.copy(), u0, X.copy(), U.copy(), diag, st))
        x = X[:, 1, :].copy()
    return out


@functools.lru_cache(maxsize=None)
def oracle_nominal(Nh, B, steps, offset, seed=SEED):
    """What an implementation that ignores the rows would compute: the oracle
    under the NOMINAL row at the own-rows loop's cold step and at its warm step
    3 (the last one of a shorter loop), from the same measured state and the
    same warm start.  {step: (u0, X, U)}."""
    cv = ffi.cfg_vector(ffi.node_config(N=Nh))
    loop = oracle_loop(Nh, B, steps, offset, True, seed)
    kp = ffi.load_params()
    out = {}
    for step in (0, min(3, steps - 1)):
        x = loop[step][0]
        X = loop[step - 1][2].copy() if step else np.zeros((B, Nh + 1, 15))
        U = loop[step - 1][3].copy() if step else np.zeros((B, Nh, 4))
        u0 = oracle_step(kp, cv, Nh, x, X, U, warm=int(step > 0))[0]
        out[step] = (u0, X, U)
    return out


def plan_gap(u0, X, U, ref):
    """Per kite, the distance of a plan (u0, trajectory, controls) to the
    reference plan `ref`, in the measure of the parity bars
    (test_gpu_parity.rel_per_kite, the largest of the three)."""
    from tests.test_gpu_parity import rel_per_kite
    return np.maximum.reduce([rel_per_kite(u0, ref[0]), rel_per_kite(X, ref[1]), rel_per_kite(U, ref[2])])
