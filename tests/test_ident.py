"""GPU tests of the aerodynamic parameter identification (k_ident_sens,
k_ident_accum, k_ident_solve) against the numpy reference on the oracle
(tests/ident_ref.py, itself checked in tests/test_ident_ref.py).

Bars: x+ 1e-12 and S 1e-10 are the project's own for the same quantities
(test_gpu_parity.rel); A, g, cost 1e-9 relative to the largest entry of each
(the 1e-10 of S, two factors and a sum).  Shapes are the smallest that reach
every edge: one, three and four items (one block, ragged), 130 (two full blocks
of 3 x 21 lanes and more), one and several substeps, whole and ragged segments
and chunks.
"""
import math

import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import FleetLoop, FlightRecorder, GpuPlant, GpuStepper
from oracle import ffi
from tests import ident_ref as ref

pytestmark = pytest.mark.gpu

H, SUB = 0.02, 2
INF = math.inf
NB = 130


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def relmax(a, b):
    """|a - b| relative to the largest entry of b."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / np.abs(b).max()


def _cfg(**kw):
    base = dict(h=H, substeps=SUB, lb_rel=INF, ub_rel=INF)
    base.update(kw)
    return ok.ident_default_config(**base)


@pytest.fixture(scope="module")
def g():
    c = ok.BatchNMPC(ok.load_properties(), ok.default_config(), 4)
    yield c
    c.close()


# ---- ident_sens ----------------------------------------------------------------
@pytest.fixture(scope="module")
def items(kp):
    rng = np.random.default_rng(31)
    x = ffi.synthetic_states(NB, offset=3100)
    u = np.column_stack([rng.uniform(0.1, 0.15, NB), rng.uniform(-0.12, 0.12, (NB, 2))])
    u[::5, 2] = 0.0                                     # rudder exactly 0 on every fifth item
    return dict(x=x, u=u, P=ok.perturb_params(kp, NB, 0.1, 32), cache={})


def _sens_ref(items, kp, substeps, shared):
    key = (substeps, shared)
    if key not in items["cache"]:
        xo = np.zeros((NB, 13)); S = np.zeros((NB, 13, 21))
        for b in range(NB):
            xo[b], S[b] = ref.sens(kp if shared else items["P"][b], items["x"][b], items["u"][b], H, substeps)
        items["cache"][key] = (xo, S)
    return items["cache"][key]


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("count", [1, 3, 4, NB])
def test_ident_sens_vs_reference(g, kp, items, count, substeps, shared):
    xr, Sr = _sens_ref(items, kp, substeps, shared)
    xo, S = g.ident_sens(items["x"][:count], items["u"][:count], H, substeps, kp if shared else items["P"][:count])
    ex, eS = rel(xo, xr[:count]), rel(S, Sr[:count])
    print(f"count {count} substeps {substeps} shared {shared}: x+ {ex:.2e}, S {eS:.2e}")
    assert ex < 1e-12 and eS < 1e-10
    rud = [ok.IDENT_FIELDS.index(f) for f in ("CYdr", "Cndr", "Cldr")]
    zero = np.flatnonzero(items["u"][:count, 2] == 0.0)
    assert zero.size and np.all(S[zero][:, :, rud] == 0.0)
    if count > 1:
        assert np.abs(S[:, :, rud]).max() > 0.0


# ---- ident_normal --------------------------------------------------------------
TLONG = 2 * ok.IDENT_CHUNK + 3          # three chunks of the kernel, the last one ragged


@pytest.fixture(scope="module")
def logs5(kp):
    B = 5
    x0 = ffi.synthetic_states(B, offset=3200)
    truth = ok.perturb_params(kp, B, 0.1, 41, fields=ok.IDENT_FIELDS)
    U = np.stack([ref.controls(TLONG, H, 50 + b) for b in range(B)])
    X = np.stack([ref.make_log(truth[b], x0[b], U[b], H, SUB) for b in range(B)])
    p21 = truth[:, ref.IDX] * (1.0 + 0.1 * np.random.default_rng(42).uniform(-1, 1, (B, 21)))
    rows = ok.perturb_params(kp, B, 0.05, 43)          # per-kite known constants and box centres
    return dict(B=B, X=X, U=U, p21=p21, rows=rows, truth=truth)


@pytest.mark.parametrize("alpha", [0.0, 100.0])
@pytest.mark.parametrize("T,L", [(1, 1), (3, 1), (7, 1), (7, 2), (7, 3), (7, 7), (TLONG, 1)])
def test_ident_normal_vs_reference(g, logs5, T, L, alpha):
    d = logs5
    cfg = _cfg(segment=L, alpha=alpha)
    X, U = d["X"][:, :T + 1].copy(), d["U"][:, :T].copy()
    A, gg, c, st = g.ident_normal(X, U, d["p21"], d["rows"], cfg)
    assert not st.any()
    worst = 0.0
    for b in range(d["B"]):
        Ar, gr, cr = ref.normal(d["rows"][b], d["p21"][b], X[b], U[b], cfg)
        assert cr > 1e-4                               # e is not small
        worst = max(worst, relmax(A[b], Ar), relmax(gg[b], gr), abs(c[b] - cr) / cr)
        assert np.array_equal(A[b], A[b].T)
    print(f"T {T} L {L} alpha {alpha}: A, g, cost vs reference {worst:.2e}")
    assert worst < 1e-9


# ---- determinism ---------------------------------------------------------------
@pytest.fixture(scope="module")
def logs130(kp):
    T = 5
    x0 = ffi.synthetic_states(NB, offset=3300)
    truth = ok.perturb_params(kp, NB, 0.1, 61, fields=ok.IDENT_FIELDS)
    U = np.stack([ref.controls(T, H, 700 + b) for b in range(NB)])
    X = np.stack([ref.make_log(truth[b], x0[b], U[b], H, SUB) for b in range(NB)])
    return dict(X=X, U=U, rows=ok.perturb_params(kp, NB, 0.05, 62), p21=truth[:, ref.IDX])


def test_a_kite_does_not_depend_on_the_batch_around_it(g, logs130):
    d = logs130
    cfg = _cfg(iters=4, segment=2)
    A, gg, c, _ = g.ident_normal(d["X"], d["U"], d["p21"], d["rows"], cfg)
    r = g.identify(d["X"], d["U"], d["rows"], cfg)
    A2, g2, c2, _ = g.ident_normal(d["X"], d["U"], d["p21"], d["rows"], cfg)
    r2 = g.identify(d["X"], d["U"], d["rows"], cfg)
    for a, b in ((A, A2), (gg, g2), (c, c2), (r.params, r2.params), (r.cost, r2.cost), (r.cost0, r2.cost0)):
        np.testing.assert_array_equal(a, b)            # two runs
    assert not (r.status & ok.IDENT_NAN).any()
    for pos in (0, 63, 64, 129):
        s = slice(pos, pos + 1)
        A1, g1, c1, _ = g.ident_normal(d["X"][s], d["U"][s], d["p21"][s], d["rows"][s], cfg)
        np.testing.assert_array_equal(A1[0], A[pos]); np.testing.assert_array_equal(g1[0], gg[pos])
        assert c1[0] == c[pos]
        r1 = g.identify(d["X"][s], d["U"][s], d["rows"][s], cfg)
        np.testing.assert_array_equal(r1.params[0], r.params[pos])
        assert (r1.cost0[0], r1.cost[0], r1.evals[0], r1.status[0]) == (r.cost0[pos], r.cost[pos], r.evals[pos],
                                                                        r.status[pos])


def test_host_and_device_entry_points_agree(g, logs130):
    d = logs130
    B, T = NB, d["U"].shape[1]
    cfg = _cfg(iters=4, segment=2)
    want = g.identify(d["X"], d["U"], d["rows"], cfg)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        X = torch.from_numpy(d["X"]).cuda(); U = torch.from_numpy(d["U"]).cuda()
        rows = torch.from_numpy(d["rows"]).cuda()
        out = torch.zeros((B, 52), dtype=torch.float64, device="cuda")
        c2 = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        ev = torch.full((B,), 77, dtype=torch.int32, device="cuda")
        st = torch.full((B,), 77, dtype=torch.int32, device="cuda")        # written, not OR-ed
        ws = torch.empty((ok.ident_workspace_doubles(cfg, B, T),), dtype=torch.float64, device="cuda")
        g.identify_device(cfg, B, T, rows.data_ptr(), B, X.data_ptr(), U.data_ptr(), out.data_ptr(), c2.data_ptr(),
                          ev.data_ptr(), st.data_ptr(), ws.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want.params)
        np.testing.assert_array_equal(c2.cpu().numpy()[:, 0], want.cost0)
        np.testing.assert_array_equal(c2.cpu().numpy()[:, 1], want.cost)
        np.testing.assert_array_equal(ev.cpu().numpy(), want.evals)
        np.testing.assert_array_equal(st.cpu().numpy(), want.status)
    finally:
        g.use_own_stream()


# ---- identify ------------------------------------------------------------------
@pytest.fixture(scope="module")
def logs4(kp):
    B, T = 4, 16
    x0 = ffi.synthetic_states(B, offset=3000)
    truth = ok.perturb_params(kp, B, 0.1, 11, fields=ok.IDENT_FIELDS)
    U = np.stack([ref.controls(T, H, 3 + b) for b in range(B)])
    X = np.stack([ref.make_log(truth[b], x0[b], U[b], H, SUB) for b in range(B)])
    return dict(B=B, T=T, X=X, U=U, truth=truth)


def _serr(rows, truth, kp):
    return np.abs((rows[:, ref.IDX] - truth[:, ref.IDX]) / ref.scales(kp)[None, :]).max(axis=1)


@pytest.mark.parametrize("L", [1, 4])
def test_identify_noiseless_recovers_the_truth(g, kp, logs4, L):
    d = logs4
    cfg = _cfg(segment=L)
    r = g.identify(d["X"], d["U"], kp, cfg)
    rr = [ref.identify(kp, d["X"][b], d["U"][b], cfg) for b in range(d["B"])]
    e_ref = _serr(np.stack([q["params"] for q in rr]), d["truth"], kp)
    e_gpu = _serr(r.params, d["truth"], kp)
    print(f"L {L}: scaled error GPU {e_gpu.max():.2e}, reference {e_ref.max():.2e}, evals {r.evals.tolist()}, "
          f"status {r.status.tolist()}")
    assert np.all(e_gpu <= np.maximum(1e-10, 1000.0 * e_ref))
    assert np.all(r.cost <= r.cost0) and np.all(r.evals <= cfg.iters)
    assert np.all(r.status & ok.IDENT_CONVERGED) and not (r.status & ok.IDENT_NAN).any()
    # everything but the 21 is the input row
    other = np.setdiff1d(np.arange(52), ref.IDX)
    np.testing.assert_array_equal(r.params[:, other], np.repeat(kp[None, other], d["B"], axis=0))


def _certificate(kp, X, U, cfg, r):
    lo, hi = -np.array(list(cfg.lb_rel)), np.array(list(cfg.ub_rel))
    s = ref.scales(kp)
    for b in range(X.shape[0]):
        z = (r.params[b, ref.IDX] - kp[ref.IDX]) / s
        _, g0, _ = ref.normal(kp, kp[ref.IDX], X[b], U[b], cfg)
        _, g1, _ = ref.normal(kp, r.params[b, ref.IDX], X[b], U[b], cfg)
        p0 = np.abs(ref.projected_gradient(np.zeros(21), g0, lo, hi)).max()
        # a variable counts as on its bound within the rounding of p = pref + s z
        zc = np.where(np.abs(z - lo) <= 1e-15 * np.maximum(1.0, np.abs(lo)), lo, z)
        zc = np.where(np.abs(z - hi) <= 1e-15 * np.maximum(1.0, np.abs(hi)), hi, zc)
        p1 = np.abs(ref.projected_gradient(zc, g1, lo, hi)).max()
        print(f"kite {b}: projected gradient {p0:.2e} -> {p1:.2e}, status {r.status[b]}")
        assert p1 <= 1e-6 * p0
        assert np.all(zc >= lo) and np.all(zc <= hi)
        on = bool(np.any((zc == lo) | (zc == hi)))
        assert on == bool(r.status[b] & ok.IDENT_AT_BOUND)
        assert not r.status[b] & ok.IDENT_NAN


def test_certificate_truth_outside_the_box(g, kp, logs4):
    """48 evaluations: every change of the active set costs the iteration a
    rejected trial or two (lambda x 8, then / 4 again), so the default 12 are not
    always enough when several of the 21 end on their bounds.  The reference
    needs 8, 17, 13 and 24 evaluations on these four logs (after 12 its kite 1
    still has a projected gradient of 1.1e-3, and so has the GPU's); 48 is twice
    its largest count."""
    d = logs4
    cfg = _cfg(lb_rel=0.05, ub_rel=0.05, iters=48)
    r = g.identify(d["X"], d["U"], kp, cfg)
    print(f"evals {r.evals.tolist()}")
    _certificate(kp, d["X"], d["U"], cfg, r)
    assert np.all(r.status & ok.IDENT_AT_BOUND) and np.all(r.status & ok.IDENT_CONVERGED)
    assert np.all(r.cost <= r.cost0)


def test_certificate_noisy_log(g, kp):
    B, T = 4, 40
    x0 = ffi.synthetic_states(B, offset=3000)
    truth = ok.perturb_params(kp, B, 0.1, 14, fields=ok.IDENT_FIELDS)
    U = np.stack([ref.controls(T, H, 6 + b) for b in range(B)])
    X = np.stack([ref.make_log(truth[b], x0[b], U[b], H, SUB) for b in range(B)])
    X = X + 1e-3 * np.random.default_rng(7).normal(size=X.shape)
    for L in (1, 4):
        cfg = _cfg(lb_rel=0.5, ub_rel=0.5, segment=L)
        _certificate(kp, X, U, cfg, g.identify(X, U, kp, cfg))


# ---- containment and validation --------------------------------------------------
def test_a_non_finite_kite_is_contained(g, kp, logs5):
    d = logs5
    T = 7
    X, U = d["X"][:, :T + 1].copy(), d["U"][:, :T].copy()
    cfg = _cfg(iters=5)
    keep = [0, 1, 3, 4]
    clean = g.identify(X[keep], U[keep], d["rows"][keep], cfg)
    assert not (clean.status & ok.IDENT_NAN).any()
    Xb = X.copy(); Xb[2, 3, 5] = np.nan                 # a NaN in kite 2's log
    r = g.identify(Xb, U, d["rows"], cfg)
    assert r.status[2] == ok.IDENT_NAN and r.params[2].tobytes() == d["rows"][2].tobytes()
    np.testing.assert_array_equal(r.params[keep], clean.params)
    np.testing.assert_array_equal(r.status[keep], clean.status)
    np.testing.assert_array_equal(r.cost[keep], clean.cost)
    Ub = U.copy(); Ub[2, 0, 1] = np.inf
    r = g.identify(X, Ub, d["rows"], cfg)
    assert r.status[2] == ok.IDENT_NAN and r.params[2].tobytes() == d["rows"][2].tobytes()
    np.testing.assert_array_equal(r.params[keep], clean.params)
    P = d["rows"].copy(); P[2, nmpc._PARAM_FIELDS.index("Cmq")] = np.nan   # a NaN in kite 2's row
    r = g.identify(X, U, P, cfg)
    assert r.status[2] == ok.IDENT_NAN and r.params[2].tobytes() == P[2].tobytes()
    np.testing.assert_array_equal(r.params[keep], clean.params)
    np.testing.assert_array_equal(r.status[keep], clean.status)
    # the status is written on every call
    again = g.identify(X, U, d["rows"], cfg)
    assert not (again.status & ok.IDENT_NAN).any()
    np.testing.assert_array_equal(again.params[keep], clean.params)


def test_bad_arguments_are_refused(g, kp, logs5):
    d = logs5
    T = 7
    X, U = d["X"][:, :T + 1].copy(), d["U"][:, :T].copy()

    def refused(call, *a, **k):
        with pytest.raises(ok.KiteNmpcError) as e:
            call(*a, **k)
        assert e.value.code == nmpc.KITE_EINVAL

    for bad in (dict(substeps=0), dict(substeps=65), dict(segment=0), dict(segment=T + 1), dict(iters=0),
                dict(iters=65), dict(h=0.0), dict(h=-0.02), dict(h=np.nan), dict(h=np.inf), dict(alpha=-1.0),
                dict(alpha=np.nan), dict(lm0=-1e-6), dict(lm0=np.inf), dict(tol=-1.0), dict(tol=np.nan),
                dict(Q=[1.0] * 12 + [-1.0]), dict(Q=[np.inf] + [1.0] * 12)):
        refused(g.identify, X, U, d["rows"], _cfg(**bad))
        refused(g.ident_normal, X, U, d["p21"], d["rows"], _cfg(**bad))
    refused(ok.ident_workspace_doubles, _cfg(), 4, 0)
    refused(ok.ident_workspace_doubles, _cfg(), 4, (1 << 20) + 1)
    P = d["rows"].copy(); P[1, nmpc._PARAM_FIELDS.index("mass")] = 0.0    # finite, but no model
    refused(g.identify, X, U, P, _cfg())
    refused(g.ident_sens, X[:, 0], U[:, 0], H, 0, d["rows"])
    refused(g.ident_sens, X[:, 0], U[:, 0], 0.0, 2, d["rows"])
    refused(g.ident_sens, X[:, 0], U[:, 0], H, 2, P)


# ---- closed loop -------------------------------------------------------------------
def _fly(nk, steps, plant_rows, recorder):
    from bench import synthetic_x0
    cfg = ok.default_config(N=20)
    h, psteps, sub = cfg.dt / 2, 2, 2
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    try:
        ctx.plant_set_params(plant_rows)
        x_init = synthetic_x0(nk, 0, ctx)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        kw = {} if recorder is None else dict(recorder=recorder)
        loop = FleetLoop(GpuStepper(ctx), torch.from_numpy(x_init).cuda(), 20, cfg.dt,
                         plant=GpuPlant(ctx, h, psteps, sub), **kw)
        u = []
        for _ in range(steps):
            loop.step()
            u.append(loop.u0.cpu().numpy().copy())
        out = None
        if recorder is not None:
            # the plant's 21 are drawn +-10 % around the nominal row: a box that holds the draw
            # (the reference's default allows CLa_total only -5 %)
            icfg = ok.ident_default_config(h=cfg.dt, substeps=psteps * sub, lb_rel=0.5, ub_rel=0.5)
            res = recorder.identify(ctx, icfg)
            torch.cuda.synchronize()
            A, _, _, _ = ctx.ident_normal(recorder.X.cpu().numpy(), recorder.U.cpu().numpy(),
                                          np.repeat(ctx.params.as_array()[None, ref.IDX], nk, axis=0), None, icfg)
            out = [t.cpu().numpy() for t in res] + [A]
        return np.stack(u), loop.x0.cpu().numpy(), out
    finally:
        ctx.close()


def test_closed_loop_identification(kp):
    nk, T = 8, 24
    plant = ok.perturb_params(kp, nk, 0.1, 71, fields=ok.IDENT_FIELDS)
    rec = FlightRecorder(nk, T, "cuda")
    u_rec, x_rec, (rows, cost2, evals, status, A) = _fly(nk, T + 1, plant, rec)
    assert rec.full
    u_plain, x_plain, _ = _fly(nk, T + 1, plant, None)
    np.testing.assert_array_equal(u_rec, u_plain)       # the recorder changes nothing
    np.testing.assert_array_equal(x_rec, x_plain)
    np.testing.assert_array_equal(rec.U.cpu().numpy(), np.transpose(u_rec[:T, :, :3], (1, 0, 2)))
    assert not (status & ok.IDENT_NAN).any()
    s = ref.scales(kp)
    for b in range(nk):
        dead = np.diag(A[b]) == 0.0                     # parameters the loop did not excite
        assert rows[b, ref.IDX[dead]].tobytes() == kp[ref.IDX[dead]].tobytes()
        e_id = np.linalg.norm(((rows[b] - plant[b])[ref.IDX] / s)[~dead])
        e_nom = np.linalg.norm(((kp - plant[b])[ref.IDX] / s)[~dead])
        print(f"kite {b}: scaled distance to the plant's 21: nominal {e_nom:.3e}, identified {e_id:.3e}, "
              f"cost {cost2[b, 0]:.2e} -> {cost2[b, 1]:.2e}, evals {evals[b]}, status {status[b]}")
        assert e_id < e_nom
        assert cost2[b, 1] <= cost2[b, 0]
