"""GPU tests of the joint identification of the 21 coefficients and a constant
wind offset per kite (k_ident_sens_jw, k_ident_accum_jw, k_ident_solve24;
kite_nmpc_ident_sens_joint, _ident_normal_joint, _identify_joint[_device])
against the numpy reference on the oracle (tests/ident_joint_ref.py, itself
checked in tests/test_ident_joint_ref.py).

Bars.  Columns, rows and sums of the 21: the project's bars of
tests/test_ident_wind.py (x+ 1e-12, S 1e-10, A, g and cost 1e-9 relative to the
largest entry of each).  Everything that involves the wind columns is compared
with a reference whose d f / d W is a Richardson-extrapolated central
difference: its bar is 10 x the reference's own propagated error estimate
(``ident_joint_ref``: E, EA, Eg), relative to the same largest entry, with a
floor of 1e-10.  The wind columns are also bracketed without that reference, by
central differences of k_ident_sens_w's x+ over the wind at two steps.
The identification: distance from the truth at most 10 x the reference's on the
same log or 1e-10, whichever is larger; all converged within 16 evaluations.

Measured on gfx950 (DESIGN.md section 4.14 has the full record): x+ 2.0e-16,
S[:, :21] 8.0e-15, wind columns 2.5e-13 at bars of 5.0e-7 .. 8.9e-7; A, g, cost
of the 21 5.0e-15, wind rows and columns 2.4e-13 at bars of 1.9e-6 .. 2.0e-2
(the bar, the plain central difference's own error carried through |df/dx|,
overstates the extrapolated reference's error by many orders: the achieved
figure is what to read); fixture J: the 21 2.0e-12 .. 4.0e-10 (reference
2.2e-12 .. 4.0e-10), wind 7.5e-15 .. 1.3e-12 m/s, 10 .. 12 evaluations; closed
loop: the 21 7.5e-13 .. 6.3e-11, wind 8.9e-16 .. 3.7e-14 m/s.
"""
import math

import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import FleetLoop, FlightRecorder, GpuPlant, GpuStepper
from oracle import ffi
from tests import ident_joint_ref as jref
from tests import ident_ref as ref
from tests import ident_wind_ref as wref

pytestmark = pytest.mark.gpu

H, SUB = 0.02, 2
INF = math.inf
NB = 130
ITERS = 16
RUD = [ok.IDENT_FIELDS.index(f) for f in ("CYdr", "Cndr", "Cldr")]


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def relmax(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / np.abs(b).max()


def _cfg(**kw):
    base = dict(h=H, substeps=SUB, lb_rel=INF, ub_rel=INF)
    base.update(kw)
    return ok.ident_default_config(**base)


def cfg_j(**kw):
    """The settings of fixture J (tests/test_ident_joint_ref.py)."""
    base = dict(h=H, substeps=SUB, lb_rel=0.5, ub_rel=0.5, lm0=1e-3, tol=1e-9, Q=[1.0] * 13, iters=ITERS)
    base.update(kw)
    return ok.ident_default_config(**base)


def _wc(**kw):
    return ok.ident_wind_default_config(**kw)


def _wref(wc):
    return jref.WindCfg(wc.w_scale, list(wc.w_prior), list(wc.w_box), wc.alpha_w)


@pytest.fixture(scope="module")
def g():
    c = ok.BatchNMPC(ok.load_properties(), ok.default_config(), 4)
    yield c
    c.close()


def _device_identify(g, cfg, wc, rows, X, U, W0=None):
    """identify_joint_device on torch tensors -> an IdentResult on the host."""
    B, T = U.shape[0], U.shape[1]
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        dX = torch.from_numpy(np.ascontiguousarray(X)).cuda(); dU = torch.from_numpy(np.ascontiguousarray(U)).cuda()
        dW = torch.from_numpy(np.ascontiguousarray(W0)).cuda() if W0 is not None else None
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, 52))
        dR = torch.from_numpy(rows).cuda()
        out = torch.zeros((B, 52), dtype=torch.float64, device="cuda")
        wo = torch.full((B, 3), 77.0, dtype=torch.float64, device="cuda")
        c2 = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        ev = torch.full((B,), 77, dtype=torch.int32, device="cuda")
        st = torch.full((B,), 77, dtype=torch.int32, device="cuda")        # written, not OR-ed
        ws = torch.empty((ok.ident_joint_workspace_doubles(cfg, B, T),), dtype=torch.float64, device="cuda")
        g.identify_joint_device(cfg, wc, B, T, dR.data_ptr(), rows.shape[0], dX.data_ptr(), dU.data_ptr(),
                                out.data_ptr(), wo.data_ptr(), c2.data_ptr(), ev.data_ptr(), st.data_ptr(),
                                ws.data_ptr(), wind0=dW.data_ptr() if dW is not None else 0)
        torch.cuda.synchronize()
        c2h = c2.cpu().numpy()
        return nmpc.IdentResult(out.cpu().numpy(), c2h[:, 0].copy(), c2h[:, 1].copy(), ev.cpu().numpy(),
                                st.cpu().numpy(), wo.cpu().numpy())
    finally:
        g.use_own_stream()


def _same(a, b):
    for f in ("params", "wind", "cost0", "cost", "evals", "status"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


# ---- 1. exports and argument rules -----------------------------------------------
@pytest.fixture(scope="module")
def logs5(kp):
    B, TL = 5, 2 * ok.IDENT_CHUNK + 3
    rng = np.random.default_rng(240)
    x0 = ffi.synthetic_states(B, offset=3200)
    truth = ok.perturb_params(kp, B, 0.1, 241, fields=ok.IDENT_FIELDS)
    U = np.stack([ref.controls(TL, H, 250 + b) for b in range(B)])
    t = np.arange(TL)[None, :, None] * H
    W = rng.uniform(-1.0, 1.0, (B, 1, 3)) + rng.uniform(-0.5, 0.5, (B, 1, 3)) * np.sin(
        2 * np.pi * 1.5 * t + rng.uniform(0, 6.28, (B, 1, 3)))
    w = rng.uniform(-0.8, 0.8, (B, 3))                   # the offset the evaluations are made at
    X = np.stack([wref.make_log(truth[b], x0[b], U[b], W[b] + 0.5 * w[b], H, SUB) for b in range(B)])
    p21 = truth[:, ref.IDX] * (1.0 + 0.1 * np.random.default_rng(242).uniform(-1, 1, (B, 21)))
    rows = ok.perturb_params(kp, B, 0.05, 243)
    return dict(B=B, X=X, U=U, W=W, w=w, p21=p21, rows=rows, truth=truth, cache={})


def test_exports_and_argument_rules(g, logs5):
    L = ok.lib()
    for n in ("kite_nmpc_ident_sens_joint", "kite_nmpc_ident_normal_joint", "kite_nmpc_identify_joint",
              "kite_nmpc_identify_joint_device", "kite_nmpc_ident_joint_workspace_doubles"):
        assert hasattr(L, n), n
    assert L.kite_nmpc_api_version() == 7
    d = logs5
    T = 7
    X, U, W = d["X"][:, :T + 1].copy(), d["U"][:, :T].copy(), d["W"][:, :T].copy()

    def refused(call, *a, **k):
        with pytest.raises(ok.KiteNmpcError) as e:
            call(*a, **k)
        assert e.value.code == nmpc.KITE_EINVAL

    # the rules of the _wind entries
    for bad in (dict(substeps=0), dict(substeps=65), dict(segment=0), dict(segment=T + 1), dict(iters=0),
                dict(iters=65), dict(h=0.0), dict(h=-0.02), dict(h=np.nan), dict(h=np.inf), dict(alpha=-1.0),
                dict(alpha=np.nan), dict(lm0=-1e-6), dict(lm0=np.inf), dict(tol=-1.0), dict(tol=np.nan),
                dict(Q=[1.0] * 12 + [-1.0]), dict(Q=[np.inf] + [1.0] * 12)):
        refused(g.identify_joint, X, U, d["rows"], _cfg(**bad), _wc(), wind0=W)
        refused(g.ident_normal_joint, X, U, d["p21"], d["w"], d["rows"], _cfg(**bad), _wc(), wind0=W)
        with pytest.raises(ok.KiteNmpcError):
            ok.ident_joint_workspace_doubles(_cfg(**bad), d["B"], T)
    P = d["rows"].copy(); P[1, nmpc._PARAM_FIELDS.index("mass")] = 0.0    # finite, but no model
    refused(g.identify_joint, X, U, P, _cfg(), _wc())
    refused(g.ident_sens_joint, X[:, 0], U[:, 0], d["w"], H, 0, d["rows"])
    refused(g.ident_sens_joint, X[:, 0], U[:, 0], d["w"], 0.0, 2, d["rows"])
    refused(g.ident_sens_joint, X[:, 0], U[:, 0], d["w"], H, 2, P)
    # the wind configuration
    B = d["B"]
    dX = torch.from_numpy(X).cuda(); dU = torch.from_numpy(U).cuda(); dR = torch.from_numpy(d["rows"]).cuda()
    out = torch.zeros((B, 52), dtype=torch.float64, device="cuda"); wo = torch.zeros((B, 3), dtype=torch.float64,
                                                                                     device="cuda")
    ws = torch.empty((ok.ident_joint_workspace_doubles(_cfg(), B, T),), dtype=torch.float64, device="cuda")
    for bad in (dict(w_scale=0.0), dict(w_scale=-1.0), dict(w_scale=np.nan), dict(w_scale=np.inf),
                dict(w_box=-1.0), dict(w_box=[3.0, np.nan, 3.0]), dict(alpha_w=-1.0), dict(alpha_w=np.nan),
                dict(alpha_w=np.inf), dict(w_prior=[0.0, np.nan, 0.0]), dict(w_prior=[np.inf, 0.0, 0.0])):
        refused(g.identify_joint, X, U, d["rows"], _cfg(), _wc(**bad))
        refused(g.ident_normal_joint, X, U, d["p21"], d["w"], d["rows"], _cfg(), _wc(**bad))
        out.fill_(5.0)
        refused(g.identify_joint_device, _cfg(), _wc(**bad), B, T, dR.data_ptr(), B, dX.data_ptr(), dU.data_ptr(),
                out.data_ptr(), wo.data_ptr(), 0, 0, 0, ws.data_ptr())
        torch.cuda.synchronize()
        assert bool((out == 5.0).all())                 # nothing was launched
    # +INFINITY is a free wind, and the device entry needs its pointers
    r = g.identify_joint(X, U, d["rows"], _cfg(iters=2), _wc(w_box=INF))
    assert not (r.status & ok.IDENT_NAN).any()
    refused(g.identify_joint_device, _cfg(), _wc(), B, T, 0, B, 0, 0, 0, 0, 0, 0, 0, 0)
    refused(g.identify_joint_device, _cfg(), _wc(), B, T, dR.data_ptr(), B, dX.data_ptr(), dU.data_ptr(),
            out.data_ptr(), 0, 0, 0, 0, ws.data_ptr())


# ---- 2. ident_sens_joint -----------------------------------------------------------
@pytest.fixture(scope="module")
def items(kp):
    rng = np.random.default_rng(231)
    x = ffi.synthetic_states(NB, offset=3100)
    u = np.column_stack([rng.uniform(0.1, 0.15, NB), rng.uniform(-0.12, 0.12, (NB, 2))])
    u[::5, 2] = 0.0                                     # rudder exactly 0 on every fifth item
    w = rng.uniform(-1.5, 1.5, (NB, 3))
    return dict(x=x, u=u, w=w, P=ok.perturb_params(kp, NB, 0.1, 232), cache={})


def _sens_ref(items, substeps):
    if substeps not in items["cache"]:
        xo = np.zeros((NB, 13)); S = np.zeros((NB, 13, 24)); E = np.zeros((NB, 13, 3))
        for b in range(NB):
            xo[b], S[b], E[b] = jref.sens(items["P"][b], items["x"][b], items["u"][b], items["w"][b], H, substeps)
        items["cache"][substeps] = (xo, S, E)
    return items["cache"][substeps]


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("count", [1, 2, 3, NB])
def test_ident_sens_joint_vs_reference(g, items, count, substeps):
    xr, Sr, Er = (a[:count] for a in _sens_ref(items, substeps))
    x, u, w, P = (items[k][:count] for k in ("x", "u", "w", "P"))
    xo, S = g.ident_sens_joint(x, u, w, H, substeps, P)
    assert S.shape == (count, 13, 24)
    ex, eS = rel(xo, xr), rel(S[:, :, :21], Sr[:, :, :21])
    xw, Sw = g.ident_sens(x, u, H, substeps, P, wind=w)
    ew21 = rel(S[:, :, :21], Sw)
    den = max(1.0, np.abs(Sr[:, :, 21:]).max())
    eW = np.abs(S[:, :, 21:] - Sr[:, :, 21:]).max() / den
    bar = max(1e-10, 10.0 * Er.max() / den)
    print(f"count {count} substeps {substeps}: x+ {ex:.2e}, S[:, :21] {eS:.2e} (vs ident_sens_wind {ew21:.2e}, "
          f"x+ bitwise {np.array_equal(xo, xw)}), wind columns {eW:.2e} at a bar of {bar:.2e} "
          f"(largest wind column entry {np.abs(Sr[:, :, 21:]).max():.2e})")
    assert ex < 1e-12 and eS < 1e-10 and ew21 < 1e-10 and rel(xo, xw) < 1e-12
    assert eW <= bar
    zero = np.flatnonzero(u[:, 2] == 0.0)
    assert zero.size and np.all(S[zero][:, :, RUD] == 0.0)
    if count > 1:
        assert np.abs(S[:, :, RUD]).max() > 0.0
    # independent of the reference's finite difference: central differences of
    # k_ident_sens_w's x+ over the wind at d and 2 d.  D(d) = S + c d^2 + O(d^4),
    # so S lies within |D(2d) - D(d)| of D(d); the rounding of a difference of
    # x+ (|x+| eps / d) is far below the floor
    d1 = 1e-3
    for i in range(3):
        D = []
        for dd in (d1, 2 * d1):
            wp, wm = w.copy(), w.copy()
            wp[:, i] += dd; wm[:, i] -= dd
            xp, _ = g.ident_sens(x, u, H, substeps, P, wind=wp)
            xm, _ = g.ident_sens(x, u, H, substeps, P, wind=wm)
            D.append((xp - xm) / (wp[:, i] - wm[:, i])[:, None])
        spread = np.abs(D[1] - D[0])
        floor = 1e-9 * max(1.0, np.abs(xo).max())
        assert np.all(np.abs(S[:, :, 21 + i] - D[0]) <= spread + floor), (i, np.abs(S[:, :, 21 + i] - D[0]).max())
        assert spread.max() < 1e-3 * den


# ---- 3. ident_normal_joint -------------------------------------------------------
def _normal_ref(d, T, L, with_w0):
    key = (T, L, with_w0)
    if key not in d["cache"]:
        cfg = _cfg(segment=L)
        d["cache"][key] = [jref.normal(d["rows"][b], d["p21"][b], d["w"][b], d["X"][b, :T + 1], d["U"][b, :T],
                                       d["W"][b, :T] if with_w0 else None, cfg, jref.WindCfg(), sums=True)
                           for b in range(3)]
    return d["cache"][key]


@pytest.mark.parametrize("with_w0", [False, True])
@pytest.mark.parametrize("alpha,alpha_w", [(0.0, 0.0), (100.0, 0.0), (0.0, 10.0), (100.0, 10.0)])
@pytest.mark.parametrize("T,L", [(1, 1), (3, 1), (3, 2), (7, 2), (7, 7), (19, 1), (19, 2), (19, 7)])
def test_ident_normal_joint_vs_reference(g, logs5, T, L, alpha, alpha_w, with_w0):
    d = logs5
    B = 3
    cfg, wc = _cfg(segment=L, alpha=alpha), _wc(alpha_w=alpha_w)
    X, U = d["X"][:B, :T + 1].copy(), d["U"][:B, :T].copy()
    W0 = d["W"][:B, :T].copy() if with_w0 else None
    A, gg, c, st = g.ident_normal_joint(X, U, d["p21"][:B], d["w"][:B], d["rows"][:B], cfg, wc, wind0=W0)
    assert A.shape == (B, 24, 24) and not st.any()
    sums = _normal_ref(d, T, L, with_w0)
    w21 = wA = wg = bA = bg = 0.0
    for b in range(B):
        Ar, gr, cr, EA, Eg = jref.finish(sums[b], alpha, alpha_w)
        assert cr > 1e-6
        assert np.array_equal(A[b], A[b].T)
        w21 = max(w21, relmax(A[b, :21, :21], Ar[:21, :21]), relmax(gg[b, :21], gr[:21]), abs(c[b] - cr) / cr)
        m = np.ones((24, 24), bool); m[:21, :21] = False
        dA, dg = np.abs(Ar[m]).max(), np.abs(gr[21:]).max()
        eA, eg = np.abs(A[b] - Ar)[m].max() / dA, np.abs(gg[b, 21:] - gr[21:]).max() / dg
        barA, barg = max(1e-10, 10.0 * EA.max() / dA), max(1e-10, 10.0 * Eg.max() / dg)
        assert eA <= barA and eg <= barg, (b, eA, barA, eg, barg)
        wA, wg, bA, bg = max(wA, eA), max(wg, eg), max(bA, barA), max(bg, barg)
    print(f"T {T} L {L} alpha {alpha} alpha_w {alpha_w} W0 {with_w0}: 21-block, g[:21], cost {w21:.2e}; wind rows "
          f"and columns of A {wA:.2e} (bar <= {bA:.2e}), of g {wg:.2e} (bar <= {bg:.2e})")
    assert w21 < 1e-9
    # at w = 0 the 21-block and the cost are those of the logged-wind entry on the same W0
    # (separate compilations of the body: parity bars, not bitwise)
    Wz = W0 if with_w0 else np.zeros((B, T, 3))
    A0, g0, c0, _ = g.ident_normal_joint(X, U, d["p21"][:B], np.zeros((B, 3)), d["rows"][:B], cfg, wc, wind0=W0)
    Aw, gw, cw, _ = g.ident_normal(X, U, d["p21"][:B], d["rows"][:B], cfg, wind=Wz)
    par = max(relmax(A0[:, :21, :21], Aw), relmax(g0[:, :21], gw), relmax(c0, cw))
    print(f"   w = 0 against ident_normal_wind: {par:.2e} (bitwise {np.array_equal(A0[:, :21, :21], Aw)})")
    assert par < 1e-9
    # a wind offset that is silently ignored would give the same evaluation
    assert relmax(A0, A) > 1e-6 or relmax(c0, c) > 1e-6


# ---- 4. identify_joint on fixture J ----------------------------------------------
CASES = [(8, 1), (16, 4), (19, 7)]


@pytest.fixture(scope="module")
def fix_j(kp):
    out = {}
    for T, L in CASES:
        d = jref.fixture_j(kp, T, H, SUB)
        cfg = cfg_j(segment=L)
        d["ref"] = [jref.identify(kp, d["X"][b], d["U"][b], None, cfg, jref.WindCfg()) for b in range(4)]
        out[T] = d
    return out


def _errs(params, wind, d, kp):
    e = np.array([jref.errors(params[b], wind[b], d["truth"][b], d["w"][b], kp) for b in range(len(wind))])
    return e[:, 0], e[:, 1]


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("T,L", CASES)
def test_identify_joint_on_fixture_j(g, kp, fix_j, T, L, entry):
    d = fix_j[T]
    cfg, wc = cfg_j(segment=L), _wc()
    if entry == "host":
        r = g.identify_joint(d["X"], d["U"], kp, cfg, wc)
    else:
        r = _device_identify(g, cfg, wc, kp, d["X"], d["U"])
    e21r, ewr = _errs(np.stack([q["params"] for q in d["ref"]]), np.stack([q["wind"] for q in d["ref"]]), d, kp)
    e21, ew = _errs(r.params, r.wind, d, kp)
    print(f"T {T} L {L} {entry}: scaled error of the 21 GPU {e21.tolist()} reference {e21r.tolist()}; wind error "
          f"[m/s] GPU {ew.tolist()} reference {ewr.tolist()}; evals GPU {r.evals.tolist()} reference "
          f"{[q['evals'] for q in d['ref']]}, status {r.status.tolist()}")
    assert np.all(r.status == ok.IDENT_CONVERGED) and np.all(r.evals <= ITERS)
    assert np.all(e21 <= np.maximum(1e-10, 10.0 * e21r)) and np.all(ew <= np.maximum(1e-10, 10.0 * ewr))
    assert np.all(r.cost <= r.cost0)
    other = np.setdiff1d(np.arange(52), ref.IDX)        # everything but the 21 is the input row
    np.testing.assert_array_equal(r.params[:, other], np.repeat(kp[None, other], 4, axis=0))


@pytest.mark.parametrize("T,L", CASES)
def test_what_the_wind_unknowns_are_for(g, kp, fix_j, T, L):
    d = fix_j[T]
    cfg = cfg_j(segment=L)
    Wt = np.repeat(d["w"][:, None], T, axis=1)
    # the same logs under a zero wind log: the wind goes into the coefficients
    r0 = g.identify(d["X"], d["U"], kp, cfg, wind=np.zeros((4, T, 3)))
    e0, _ = _errs(r0.params, d["w"], d, kp)
    enom, _ = _errs(np.repeat(kp[None], 4, axis=0), d["w"], d, kp)
    print(f"T {T} L {L}: identify_wind with W0 = 0 ends {e0.tolist()} from the truth (nominal row: {enom.tolist()})")
    assert np.all(e0 > 1e-3)
    # the wind known and its box closed: the logged-wind identification.  The two
    # iterations are not the same one: the joint damping is lambda tr(A) / 24 over
    # 24 diagonal entries, so the iterates differ and each run stops wherever its
    # own step first falls below tol.  Two runs stopped at tol = 1e-9 are each
    # within about tol of the common optimum, not within 1e-10 of each other
    # (measured on gfx950 with tol = 1e-9: 1.2e-11 at (8, 1), 6.6e-10 at (16, 4)).
    # The 1e-10 parity bar is therefore taken where both have converged beyond
    # it: tol = 1e-12, same logs, same 16 evaluations.
    cfg = cfg_j(segment=L, tol=1e-12)
    rw = g.identify(d["X"], d["U"], kp, cfg, wind=Wt)
    rj = g.identify_joint(d["X"], d["U"], kp, cfg, _wc(w_box=0.0), wind0=Wt)
    par = np.abs((rj.params - rw.params)[:, ref.IDX] / ref.scales(kp)[None, :]).max()
    print(f"   w_box = 0, W0 the true wind: the 21 against identify_wind {par:.2e}, wind {np.abs(rj.wind).max():.1e}, "
          f"status {rj.status.tolist()} / {rw.status.tolist()}, evals {rj.evals.tolist()} / {rw.evals.tolist()}")
    assert par <= 1e-10 and not rj.wind.any()
    assert not (rj.status & ok.IDENT_NAN).any() and not (rw.status & ok.IDENT_NAN).any()
    assert np.all(rj.status & ok.IDENT_WIND_AT_BOUND)    # a closed box: the wind is on it


@pytest.mark.parametrize("T,L", CASES)
def test_true_wind_outside_the_box(g, kp, fix_j, T, L):
    """The certificate of tests/test_ident.py: the reference's projected
    gradient at the GPU's point is at most 1e-6 of the one at the start."""
    d = fix_j[T]
    box = 0.1
    assert np.all(np.abs(d["w"]).max(axis=1) > 2 * box)
    cfg, wc = cfg_j(segment=L, iters=64), _wc(w_box=box)
    r = g.identify_joint(d["X"], d["U"], kp, cfg, wc)
    wr = _wref(wc)
    lo, hi = jref.bounds(cfg, wr)
    s = ref.scales(kp)
    for b in range(4):
        assert r.status[b] & ok.IDENT_WIND_AT_BOUND and not r.status[b] & ok.IDENT_NAN
        assert np.all(np.abs(r.wind[b]) <= box) and np.any(np.abs(r.wind[b]) == box)
        z = np.r_[(r.params[b, ref.IDX] - kp[ref.IDX]) / s, r.wind[b]]
        _, g0, _, _, _ = jref.normal(kp, kp[ref.IDX], np.zeros(3), d["X"][b], d["U"][b], None, cfg, wr)
        _, g1, _, _, _ = jref.normal(kp, r.params[b, ref.IDX], r.wind[b], d["X"][b], d["U"][b], None, cfg, wr)
        zc = np.where(np.abs(z - lo) <= 1e-15 * np.maximum(1.0, np.abs(lo)), lo, z)
        zc = np.where(np.abs(z - hi) <= 1e-15 * np.maximum(1.0, np.abs(hi)), hi, zc)
        p0 = np.abs(ref.projected_gradient(np.zeros(24), g0, lo, hi)).max()
        p1 = np.abs(ref.projected_gradient(zc, g1, lo, hi)).max()
        print(f"T {T} L {L} kite {b}: wind {r.wind[b].tolist()} (true {d['w'][b].tolist()}), projected gradient "
              f"{p0:.2e} -> {p1:.2e}, evals {r.evals[b]}, status {r.status[b]}")
        assert p1 <= 1e-6 * p0


# ---- 5. containment and determinism ------------------------------------------------
def test_non_finite_inputs_are_contained(g, logs5):
    d = logs5
    T = 7
    X, U, W = d["X"][:, :T + 1].copy(), d["U"][:, :T].copy(), d["W"][:, :T].copy()
    cfg, wc = _cfg(iters=5), _wc(w_prior=[0.1, -0.2, 0.3])
    keep = [0, 1, 3, 4]
    clean = g.identify_joint(X[keep], U[keep], d["rows"][keep], cfg, wc, wind0=W[keep])
    assert not (clean.status & ok.IDENT_NAN).any()
    Wb = W.copy(); Wb[2, 3, 1] = np.nan                 # in kite 2's W0
    Xb = X.copy(); Xb[2, 4, 6] = np.inf                 # in its log
    Pb = d["rows"].copy(); Pb[2, ref.IDX[3]] = np.nan   # in its row
    for name, (Xi, Wi, Pi) in dict(W0=(X, Wb, d["rows"]), log=(Xb, W, d["rows"]), row=(X, W, Pb)).items():
        for r in (g.identify_joint(Xi, U, Pi, cfg, wc, wind0=Wi), _device_identify(g, cfg, wc, Pi, Xi, U, Wi)):
            assert r.status[2] == ok.IDENT_NAN, name
            assert r.params[2].tobytes() == Pi[2].tobytes() and r.wind[2].tolist() == [0.1, -0.2, 0.3], name
            for f in ("params", "wind", "status", "cost", "cost0", "evals"):
                np.testing.assert_array_equal(getattr(r, f)[keep], getattr(clean, f), err_msg=name)
        if name != "row":
            _, _, c, st = g.ident_normal_joint(Xi, U, d["p21"], d["w"], Pi, cfg, wc, wind0=Wi)
            assert st[2] == ok.IDENT_NAN and not np.isfinite(c[2]) and not st[keep].any()
    again = g.identify_joint(X, U, d["rows"], cfg, wc, wind0=W)           # the status is written on every call
    assert not (again.status & ok.IDENT_NAN).any()
    np.testing.assert_array_equal(again.params[keep], clean.params)


@pytest.fixture(scope="module")
def logs130(kp):
    T = 5
    rng = np.random.default_rng(260)
    x0 = ffi.synthetic_states(NB, offset=3300)
    truth = ok.perturb_params(kp, NB, 0.1, 261, fields=ok.IDENT_FIELDS)
    U = np.stack([ref.controls(T, H, 900 + b) for b in range(NB)])
    W = rng.uniform(-1.5, 1.5, (NB, 1, 3)) + rng.uniform(-0.3, 0.3, (NB, T, 3))
    X = np.stack([wref.make_log(truth[b], x0[b], U[b], W[b], H, SUB) for b in range(NB)])
    return dict(X=X, U=U, W=W, rows=ok.perturb_params(kp, NB, 0.05, 262), p21=truth[:, ref.IDX],
                w=rng.uniform(-0.5, 0.5, (NB, 3)))


def test_a_kite_does_not_depend_on_the_batch_around_it(g, logs130):
    d = logs130
    cfg, wc = _cfg(iters=4, segment=2), _wc()
    W0 = d["W"] - d["W"].mean(axis=1, keepdims=True)    # the gust is known, the mean wind is not
    A, gg, c, _ = g.ident_normal_joint(d["X"], d["U"], d["p21"], d["w"], d["rows"], cfg, wc, wind0=W0)
    A2, g2, c2, _ = g.ident_normal_joint(d["X"], d["U"], d["p21"], d["w"], d["rows"], cfg, wc, wind0=W0)
    for a, b in ((A, A2), (gg, g2), (c, c2)):
        np.testing.assert_array_equal(a, b)            # two runs
    r = g.identify_joint(d["X"], d["U"], d["rows"], cfg, wc, wind0=W0)
    _same(r, g.identify_joint(d["X"], d["U"], d["rows"], cfg, wc, wind0=W0))
    _same(r, _device_identify(g, cfg, wc, d["rows"], d["X"], d["U"], W0))
    assert not (r.status & ok.IDENT_NAN).any() and np.abs(r.wind).max() > 1e-3
    for pos in (0, 1, 2, 63, 64, 129):
        s = slice(pos, pos + 1)
        A1, g1, c1, _ = g.ident_normal_joint(d["X"][s], d["U"][s], d["p21"][s], d["w"][s], d["rows"][s], cfg, wc,
                                             wind0=W0[s])
        np.testing.assert_array_equal(A1[0], A[pos]); np.testing.assert_array_equal(g1[0], gg[pos])
        assert c1[0] == c[pos]
        for r1 in (g.identify_joint(d["X"][s], d["U"][s], d["rows"][s], cfg, wc, wind0=W0[s]),
                   _device_identify(g, cfg, wc, d["rows"][s], d["X"][s], d["U"][s], W0[s])):
            np.testing.assert_array_equal(r1.params[0], r.params[pos])
            np.testing.assert_array_equal(r1.wind[0], r.wind[pos])
            assert (r1.cost0[0], r1.cost[0], r1.evals[0], r1.status[0]) == (r.cost0[pos], r.cost[pos], r.evals[pos],
                                                                            r.status[pos])


# ---- 6. closed loop ------------------------------------------------------------------
class _SpyStepper(GpuStepper):
    """Records what the loop hands to kite_nmpc_set_wind_device."""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.winds = []

    def set_wind_device(self, wind, wmax):
        self.winds.append((wind.clone(), wmax))
        super().set_wind_device(wind, wmax)


def _fly(nk, steps, plant_rows, wind, mode, icfg=None):
    """mode: "plain" (no recorder), "record" (a recorder, no adaptation),
    "joint" (recorder, adapt and ident_wind="joint")."""
    from bench import synthetic_x0
    cfg = ok.default_config(N=20)
    T = steps - 1
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    try:
        ctx.plant_set_params(plant_rows)
        ctx.plant_set_wind(wind=wind)                   # constant, no gust; the controller is told nothing
        x_init = synthetic_x0(nk, 0, ctx)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        kw = {}
        rec = FlightRecorder(nk, T, "cuda") if mode != "plain" else None
        if mode == "record":
            kw = dict(recorder=rec)
        elif mode == "joint":
            kw = dict(recorder=rec, adapt=icfg, ident_wind="joint")
        stepper = _SpyStepper(ctx)
        loop = FleetLoop(stepper, torch.from_numpy(x_init).cuda(), 20, cfg.dt, plant=GpuPlant(ctx, cfg.dt, 1, SUB),
                         **kw)
        u, x = [], []
        for k in range(steps):
            loop.step()                                 # step T fills the log (its state is X[T])
            u.append(loop.u0.cpu().numpy().copy()); x.append(loop.x0.cpu().numpy().copy())
        torch.cuda.synchronize()
        out = dict(u=np.stack(u), x=np.stack(x), dt=cfg.dt)
        if mode == "record":
            assert rec.full
            out.update(X=rec.X.cpu().numpy(), U=rec.U.cpu().numpy())
        if mode == "joint":
            out.update(count=loop.adapt_count, params_status=loop.params_status.cpu().numpy(),
                       ident_status=loop.ident_status.cpu().numpy(), evals=loop.ident_evals.cpu().numpy(),
                       ident_rows=loop.ident_rows.cpu().numpy(), in_force=np.asarray(ctx.get_params()),
                       wind_est=loop.ident_wind_est.cpu().numpy(), cost2=loop.ident_cost2.cpu().numpy(),
                       handed=[(w.cpu().numpy(), m) for w, m in stepper.winds], wind_max=loop.wind_max)
        return out
    finally:
        ctx.close()


def test_closed_loop_joint_identification(g, kp):
    nk, T = 8, 24
    plant = ok.perturb_params(kp, nk, 0.1, 71, fields=ok.IDENT_FIELDS)
    wind = np.random.default_rng(72).uniform(-1.5, 1.5, (nk, 3))
    dt = ok.default_config(N=20).dt
    # lm0 = 1e-3 as on fixture J; 32 evaluations: kite 0's closed-loop log takes 24 (the
    # reference and the GPU alike; the other seven 10 to 12), and a kite that has not
    # converged when the evaluations run out keeps its row
    icfg = ok.ident_default_config(h=dt, substeps=SUB, lb_rel=0.5, ub_rel=0.5, lm0=1e-3, iters=32)
    plain = _fly(nk, T + 1, plant, wind, "plain")
    rec = _fly(nk, T + 1, plant, wind, "record")
    jo = _fly(nk, T + 1, plant, wind, "joint", icfg)
    # recorder and keyword change no control and no state before the adaptation
    np.testing.assert_array_equal(rec["u"], plain["u"]); np.testing.assert_array_equal(rec["x"], plain["x"])
    np.testing.assert_array_equal(jo["u"][:T], plain["u"][:T]); np.testing.assert_array_equal(jo["x"][:T], plain["x"][:T])
    assert jo["count"] == 1
    print(f"adapt: ident status {jo['ident_status'].tolist()}, evals {jo['evals'].tolist()}, params status "
          f"{jo['params_status'].tolist()}")
    assert np.all(jo["params_status"] == 0)
    assert np.all(jo["ident_status"] & ok.IDENT_CONVERGED) and not (jo["ident_status"] & ok.IDENT_NAN).any()
    np.testing.assert_array_equal(jo["in_force"], jo["ident_rows"])       # the controller's rows are the identified ones
    assert len(jo["handed"]) == 1
    handed, wmax = jo["handed"][0]
    np.testing.assert_array_equal(handed, jo["wind_est"]); assert wmax == jo["wind_max"]
    # against the reference on the same downloaded logs, by the rule of the fixture-J test
    X, U = rec["X"], rec["U"]
    s = ref.scales(kp)
    wr = jref.WindCfg()
    A, _, _, _ = g.ident_normal_joint(X, U, np.repeat(kp[None, ref.IDX], nk, axis=0), np.zeros((nk, 3)), kp, icfg,
                                      _wc())
    for b in range(nk):
        live = np.diag(A[b])[:21] != 0.0                # the parameters the loop excited
        q = jref.identify(kp, X[b], U[b], None, icfg, wr)
        dist = lambda row: np.abs(((row - plant[b])[ref.IDX] / s)[live]).max()
        e_gpu, e_ref, e_nom = dist(jo["ident_rows"][b]), dist(q["params"]), dist(kp)
        w_gpu, w_ref = np.abs(jo["wind_est"][b] - wind[b]).max(), np.abs(q["wind"] - wind[b]).max()
        print(f"kite {b}: scaled distance of the 21 to the plant's: nominal {e_nom:.3e}, GPU {e_gpu:.3e}, reference "
              f"{e_ref:.3e}; wind error [m/s]: told nothing {np.abs(wind[b]).max():.3e}, GPU {w_gpu:.3e}, reference "
              f"{w_ref:.3e}; evals GPU {jo['evals'][b]} reference {q['evals']}, cost {jo['cost2'][b, 0]:.2e} -> "
              f"{jo['cost2'][b, 1]:.2e}, {int(live.sum())} of 21 excited")
        assert jo["ident_rows"][b, ref.IDX[~live]].tobytes() == kp[ref.IDX[~live]].tobytes()
        assert q["status"] & ok.IDENT_CONVERGED
        assert e_gpu <= max(1e-10, 10.0 * e_ref) and w_gpu <= max(1e-10, 10.0 * w_ref)
