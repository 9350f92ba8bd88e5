"""GPU tests of the identification under a logged wind (k_ident_sens_w,
k_ident_accum_w; kite_nmpc_ident_sens_wind, _ident_normal_wind,
_identify_wind[_device]) against the numpy reference on the oracle
(tests/ident_wind_ref.py, itself checked in tests/test_ident_wind_ref.py).

Bars: those of tests/test_ident.py for the same quantities -- x+ 1e-12, S 1e-10,
A, g and cost 1e-9 relative to the largest entry of each; the wind adds a
handful of operations per stage.  The identification on fixture W
(``ident_wind_ref.fixture_w``): e_gpu <= max(1e-10, 1000 e_ref) per kite.
Shapes as in tests/test_ident.py: one, three and four items, 130 (two full
blocks of 3 x 21 lanes and more), one and several substeps, whole and ragged
segments and chunks.
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
from tests import ident_wind_ref as wref

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
    rng = np.random.default_rng(131)
    x = ffi.synthetic_states(NB, offset=3100)
    u = np.column_stack([rng.uniform(0.1, 0.15, NB), rng.uniform(-0.12, 0.12, (NB, 2))])
    u[::5, 2] = 0.0                                     # rudder exactly 0 on every fifth item
    w = rng.uniform(-1.5, 1.5, (NB, 3))
    return dict(x=x, u=u, w=w, P=ok.perturb_params(kp, NB, 0.1, 132), cache={})


def _sens_ref(items, substeps):
    if substeps not in items["cache"]:
        xo = np.zeros((NB, 13)); S = np.zeros((NB, 13, 21))
        for b in range(NB):
            xo[b], S[b] = wref.sens(items["P"][b], items["x"][b], items["u"][b], items["w"][b], H, substeps)
        items["cache"][substeps] = (xo, S)
    return items["cache"][substeps]


@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("count", [1, 3, 4, NB])
def test_ident_sens_wind_vs_reference(g, items, count, substeps):
    xr, Sr = _sens_ref(items, substeps)
    xo, S = g.ident_sens(items["x"][:count], items["u"][:count], H, substeps, items["P"][:count],
                         wind=items["w"][:count])
    ex, eS = rel(xo, xr[:count]), rel(S, Sr[:count])
    print(f"count {count} substeps {substeps}: x+ {ex:.2e}, S {eS:.2e}")
    assert ex < 1e-12 and eS < 1e-10
    rud = [ok.IDENT_FIELDS.index(f) for f in ("CYdr", "Cndr", "Cldr")]
    zero = np.flatnonzero(items["u"][:count, 2] == 0.0)
    assert zero.size and np.all(S[zero][:, :, rud] == 0.0)
    if count > 1:
        assert np.abs(S[:, :, rud]).max() > 0.0
    # the wind is seen: the windless interval differs
    x0, _ = g.ident_sens(items["x"][:count], items["u"][:count], H, substeps, items["P"][:count])
    assert rel(x0, xo) > 1e-6


# ---- ident_normal --------------------------------------------------------------
TLONG = 2 * ok.IDENT_CHUNK + 3          # 19: three chunks of the kernel, the last one ragged


@pytest.fixture(scope="module")
def logs5(kp):
    B = 5
    rng = np.random.default_rng(140)
    x0 = ffi.synthetic_states(B, offset=3200)
    truth = ok.perturb_params(kp, B, 0.1, 141, fields=ok.IDENT_FIELDS)
    U = np.stack([ref.controls(TLONG, H, 150 + b) for b in range(B)])
    t = np.arange(TLONG)[None, :, None] * H
    W = rng.uniform(-1.5, 1.5, (B, 1, 3)) + rng.uniform(-0.5, 0.5, (B, 1, 3)) * np.sin(
        2 * np.pi * 1.5 * t + rng.uniform(0, 6.28, (B, 1, 3)))
    X = np.stack([wref.make_log(truth[b], x0[b], U[b], W[b], H, SUB) for b in range(B)])
    p21 = truth[:, ref.IDX] * (1.0 + 0.1 * np.random.default_rng(142).uniform(-1, 1, (B, 21)))
    rows = ok.perturb_params(kp, B, 0.05, 143)          # per-kite known constants and box centres
    return dict(B=B, X=X, U=U, W=W, p21=p21, rows=rows, truth=truth)


@pytest.mark.parametrize("alpha", [0.0, 100.0])
@pytest.mark.parametrize("T,L", [(1, 1), (3, 1), (7, 2), (7, 7), (TLONG, 1)])
def test_ident_normal_wind_vs_reference(g, logs5, T, L, alpha):
    d = logs5
    cfg = _cfg(segment=L, alpha=alpha)
    X, U, W = d["X"][:, :T + 1].copy(), d["U"][:, :T].copy(), d["W"][:, :T].copy()
    A, gg, c, st = g.ident_normal(X, U, d["p21"], d["rows"], cfg, wind=W)
    assert not st.any()
    worst = 0.0
    for b in range(d["B"]):
        Ar, gr, cr = wref.normal(d["rows"][b], d["p21"][b], X[b], U[b], W[b], cfg)
        assert cr > 1e-4                               # e is not small
        worst = max(worst, relmax(A[b], Ar), relmax(gg[b], gr), abs(c[b] - cr) / cr)
        assert np.array_equal(A[b], A[b].T)
    print(f"T {T} L {L} alpha {alpha}: A, g, cost vs reference {worst:.2e}")
    assert worst < 1e-9
    # a wind that is silently ignored would give the windless evaluation
    A0, g0, c0, _ = g.ident_normal(X, U, d["p21"], d["rows"], cfg)
    seen = max(relmax(A0, A), relmax(g0, gg), relmax(c0, c))
    print(f"   windless evaluation of the same log differs by {seen:.2e}")
    assert seen > 1e-3


def test_a_constant_wind_broadcasts_over_the_log(g, logs5):
    d = logs5
    T = 7
    cfg = _cfg(segment=2)
    X, U = d["X"][:, :T + 1].copy(), d["U"][:, :T].copy()
    w = d["W"][:, 0].copy()
    a = g.ident_normal(X, U, d["p21"], d["rows"], cfg, wind=w)
    b = g.ident_normal(X, U, d["p21"], d["rows"], cfg, wind=np.repeat(w[:, None], T, axis=1))
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p, q)


# ---- an all-zero wind log against the windless entry ------------------------------
def test_zero_wind_log_agrees_with_the_windless_entry(g, kp):
    """With W = 0 the air-relative velocity is v exactly, value and tangent, but
    k_ident_accum_w is a separate compilation of the body, and the result is NOT
    bitwise the windless kernel's.  Measured on gfx950 on these logs: x+, S, g
    and the cost are bitwise equal; A at the nominal point differs in its
    smallest entries by <= 1.7e-18 absolute; from there the iterations part at
    rounding level and the identified 21 end 1.5e-16 (L = 1) and 4.9e-14 (L = 4)
    apart in the scaled variables.  So the two are held to the parity bars of
    this file: x+ 1e-12, S 1e-10, A, g and cost 1e-9, and the identified 21 to
    the identification's 1e-10 in the scaled variables, on windless logs that
    both recover."""
    B, T = 4, 16
    x0 = ffi.synthetic_states(B, offset=3000)
    truth = ok.perturb_params(kp, B, 0.1, 11, fields=ok.IDENT_FIELDS)
    U = np.stack([ref.controls(T, H, 3 + b) for b in range(B)])
    X = np.stack([ref.make_log(truth[b], x0[b], U[b], H, SUB) for b in range(B)])
    p21 = truth[:, ref.IDX] * (1.0 + 0.1 * np.random.default_rng(170).uniform(-1, 1, (B, 21)))
    Z = np.zeros((B, T, 3))
    for L in (1, 4):
        cfg = _cfg(segment=L)
        a = g.ident_normal(X, U, p21, kp, cfg)
        b = g.ident_normal(X, U, p21, kp, cfg, wind=Z)
        eA, eg, ec = relmax(b[0], a[0]), relmax(b[1], a[1]), relmax(b[2], a[2])
        r0 = g.identify(X, U, kp, cfg)
        r1 = g.identify(X, U, kp, cfg, wind=Z)
        ep = np.abs((r1.params - r0.params)[:, ref.IDX] / ref.scales(kp)[None, :]).max()
        print(f"L {L}: zero wind log vs windless entry: A {eA:.2e}, g {eg:.2e}, cost {ec:.2e}, identified 21 {ep:.2e} "
              f"(bitwise: normal {all(np.array_equal(p, q) for p, q in zip(a, b))}, "
              f"identify {np.array_equal(r0.params, r1.params)})")
        assert max(eA, eg, ec) < 1e-9 and ep <= 1e-10
        assert np.all(r1.status & ok.IDENT_CONVERGED) and not (r1.status & ok.IDENT_NAN).any()
    s0 = g.ident_sens(X[:, 0], U[:, 0], H, SUB, kp)
    s1 = g.ident_sens(X[:, 0], U[:, 0], H, SUB, kp, wind=Z[:, 0])
    ex, eS = rel(s1[0], s0[0]), rel(s1[1], s0[1])
    print(f"ident_sens: x+ {ex:.2e}, S {eS:.2e}")
    assert ex < 1e-12 and eS < 1e-10


# ---- identify on fixture W -------------------------------------------------------
def _serr(rows, truth, kp):
    return np.abs((rows[:, ref.IDX] - truth[:, ref.IDX]) / ref.scales(kp)[None, :]).max(axis=1)


@pytest.mark.parametrize("T,L", [(8, 1), (16, 4), (19, 7)])
def test_identify_on_fixture_w_recovers_the_truth(g, kp, T, L):
    d = wref.fixture_w(kp, T, H, SUB)
    cfg = _cfg(segment=L, iters=6)
    r = g.identify(d["X"], d["U"], kp, cfg, wind=d["W"])
    rr = [wref.identify(kp, d["X"][b], d["U"][b], d["W"][b], cfg) for b in range(4)]
    e_ref = _serr(np.stack([q["params"] for q in rr]), d["truth"], kp)
    e_gpu = _serr(r.params, d["truth"], kp)
    print(f"T {T} L {L}: scaled error GPU {e_gpu.tolist()}, reference {e_ref.tolist()}, evals {r.evals.tolist()}, "
          f"status {r.status.tolist()}")
    assert np.all(e_gpu <= np.maximum(1e-10, 1000.0 * e_ref))
    assert np.all(r.cost <= r.cost0) and np.all(r.evals <= cfg.iters)
    assert np.all(r.status & ok.IDENT_CONVERGED) and not (r.status & ok.IDENT_NAN).any()
    other = np.setdiff1d(np.arange(52), ref.IDX)        # everything but the 21 is the input row
    np.testing.assert_array_equal(r.params[:, other], np.repeat(kp[None, other], 4, axis=0))


# ---- determinism, host and device entries ----------------------------------------
@pytest.fixture(scope="module")
def logs130(kp):
    T = 5
    rng = np.random.default_rng(160)
    x0 = ffi.synthetic_states(NB, offset=3300)
    truth = ok.perturb_params(kp, NB, 0.1, 161, fields=ok.IDENT_FIELDS)
    U = np.stack([ref.controls(T, H, 800 + b) for b in range(NB)])
    W = rng.uniform(-1.5, 1.5, (NB, 1, 3)) + rng.uniform(-0.3, 0.3, (NB, T, 3))
    X = np.stack([wref.make_log(truth[b], x0[b], U[b], W[b], H, SUB) for b in range(NB)])
    return dict(X=X, U=U, W=W, rows=ok.perturb_params(kp, NB, 0.05, 162), p21=truth[:, ref.IDX])


def test_a_kite_does_not_depend_on_the_batch_around_it(g, logs130):
    d = logs130
    cfg = _cfg(iters=4, segment=2)
    A, gg, c, _ = g.ident_normal(d["X"], d["U"], d["p21"], d["rows"], cfg, wind=d["W"])
    r = g.identify(d["X"], d["U"], d["rows"], cfg, wind=d["W"])
    A2, g2, c2, _ = g.ident_normal(d["X"], d["U"], d["p21"], d["rows"], cfg, wind=d["W"])
    r2 = g.identify(d["X"], d["U"], d["rows"], cfg, wind=d["W"])
    for a, b in ((A, A2), (gg, g2), (c, c2), (r.params, r2.params), (r.cost, r2.cost), (r.cost0, r2.cost0)):
        np.testing.assert_array_equal(a, b)            # two runs
    assert not (r.status & ok.IDENT_NAN).any()
    for pos in (0, 63, 64, 129):
        s = slice(pos, pos + 1)
        A1, g1, c1, _ = g.ident_normal(d["X"][s], d["U"][s], d["p21"][s], d["rows"][s], cfg, wind=d["W"][s])
        np.testing.assert_array_equal(A1[0], A[pos]); np.testing.assert_array_equal(g1[0], gg[pos])
        assert c1[0] == c[pos]
        r1 = g.identify(d["X"][s], d["U"][s], d["rows"][s], cfg, wind=d["W"][s])
        np.testing.assert_array_equal(r1.params[0], r.params[pos])
        assert (r1.cost0[0], r1.cost[0], r1.evals[0], r1.status[0]) == (r.cost0[pos], r.cost[pos], r.evals[pos],
                                                                        r.status[pos])


def test_host_and_device_entry_points_agree(g, logs130):
    d = logs130
    B, T = NB, d["U"].shape[1]
    cfg = _cfg(iters=4, segment=2)
    want = g.identify(d["X"], d["U"], d["rows"], cfg, wind=d["W"])
    windless = g.identify(d["X"], d["U"], d["rows"], cfg)
    assert not np.array_equal(want.params, windless.params)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        X = torch.from_numpy(d["X"]).cuda(); U = torch.from_numpy(d["U"]).cuda(); W = torch.from_numpy(d["W"]).cuda()
        rows = torch.from_numpy(d["rows"]).cuda()
        out = torch.zeros((B, 52), dtype=torch.float64, device="cuda")
        c2 = torch.zeros((B, 2), dtype=torch.float64, device="cuda")
        ev = torch.full((B,), 77, dtype=torch.int32, device="cuda")
        st = torch.full((B,), 77, dtype=torch.int32, device="cuda")        # written, not OR-ed
        ws = torch.empty((ok.ident_workspace_doubles(cfg, B, T),), dtype=torch.float64, device="cuda")
        g.identify_device(cfg, B, T, rows.data_ptr(), B, X.data_ptr(), U.data_ptr(), out.data_ptr(), c2.data_ptr(),
                          ev.data_ptr(), st.data_ptr(), ws.data_ptr(), wind=W.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want.params)
        np.testing.assert_array_equal(c2.cpu().numpy()[:, 0], want.cost0)
        np.testing.assert_array_equal(c2.cpu().numpy()[:, 1], want.cost)
        np.testing.assert_array_equal(ev.cpu().numpy(), want.evals)
        np.testing.assert_array_equal(st.cpu().numpy(), want.status)
        # no wind pointer: the windless entry
        g.identify_device(cfg, B, T, rows.data_ptr(), B, X.data_ptr(), U.data_ptr(), out.data_ptr(), c2.data_ptr(),
                          ev.data_ptr(), st.data_ptr(), ws.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), windless.params)
    finally:
        g.use_own_stream()


# ---- containment and validation --------------------------------------------------
def test_a_non_finite_wind_is_contained(g, logs5):
    d = logs5
    T = 7
    X, U, W = d["X"][:, :T + 1].copy(), d["U"][:, :T].copy(), d["W"][:, :T].copy()
    cfg = _cfg(iters=5)
    keep = [0, 1, 3, 4]
    clean = g.identify(X[keep], U[keep], d["rows"][keep], cfg, wind=W[keep])
    assert not (clean.status & ok.IDENT_NAN).any()
    for bad in (np.nan, np.inf):
        Wb = W.copy(); Wb[2, 3, 1] = bad                # in kite 2's wind log
        r = g.identify(X, U, d["rows"], cfg, wind=Wb)
        assert r.status[2] == ok.IDENT_NAN and r.params[2].tobytes() == d["rows"][2].tobytes()
        for f in ("params", "status", "cost", "cost0", "evals"):
            np.testing.assert_array_equal(getattr(r, f)[keep], getattr(clean, f))
        _, _, c, st = g.ident_normal(X, U, d["p21"], d["rows"], cfg, wind=Wb)
        assert st[2] == ok.IDENT_NAN and not np.isfinite(c[2]) and not st[keep].any()
    again = g.identify(X, U, d["rows"], cfg, wind=W)    # the status is written on every call
    assert not (again.status & ok.IDENT_NAN).any()
    np.testing.assert_array_equal(again.params[keep], clean.params)


def test_bad_arguments_are_refused(g, logs5):
    d = logs5
    T = 7
    X, U, W = d["X"][:, :T + 1].copy(), d["U"][:, :T].copy(), d["W"][:, :T].copy()

    def refused(call, *a, **k):
        with pytest.raises(ok.KiteNmpcError) as e:
            call(*a, **k)
        assert e.value.code == nmpc.KITE_EINVAL

    for bad in (dict(substeps=0), dict(substeps=65), dict(segment=0), dict(segment=T + 1), dict(iters=0),
                dict(iters=65), dict(h=0.0), dict(h=-0.02), dict(h=np.nan), dict(h=np.inf), dict(alpha=-1.0),
                dict(alpha=np.nan), dict(lm0=-1e-6), dict(lm0=np.inf), dict(tol=-1.0), dict(tol=np.nan),
                dict(Q=[1.0] * 12 + [-1.0]), dict(Q=[np.inf] + [1.0] * 12)):
        refused(g.identify, X, U, d["rows"], _cfg(**bad), wind=W)
        refused(g.ident_normal, X, U, d["p21"], d["rows"], _cfg(**bad), wind=W)
    P = d["rows"].copy(); P[1, nmpc._PARAM_FIELDS.index("mass")] = 0.0    # finite, but no model
    refused(g.identify, X, U, P, _cfg(), wind=W)
    refused(g.ident_sens, X[:, 0], U[:, 0], H, 0, d["rows"], wind=W[:, 0])
    refused(g.ident_sens, X[:, 0], U[:, 0], 0.0, 2, d["rows"], wind=W[:, 0])
    refused(g.ident_sens, X[:, 0], U[:, 0], H, 2, P, wind=W[:, 0])
    # the device entry: a missing log or workspace
    B = d["B"]
    Wd = torch.from_numpy(W).cuda()
    refused(g.identify_device, _cfg(), B, T, 0, B, 0, 0, 0, 0, 0, 0, 0, wind=Wd.data_ptr())


# ---- closed loop -------------------------------------------------------------------
def _fly(nk, steps, plant_rows, wind, recorder, adapt=None):
    from bench import synthetic_x0
    cfg = ok.default_config(N=20)
    h, psteps, sub = cfg.dt / 2, 2, 2
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    try:
        ctx.plant_set_params(plant_rows)
        ctx.plant_set_wind(wind=wind)                   # constant, no gust
        ctx.set_wind(wind)                              # the controller is told the same wind
        x_init = synthetic_x0(nk, 0, ctx)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        kw = {}
        if recorder is not None:
            kw = dict(recorder=recorder, ident_wind=torch.from_numpy(wind).cuda())
            if adapt is not None:
                kw["adapt"] = adapt
        loop = FleetLoop(GpuStepper(ctx), torch.from_numpy(x_init).cuda(), 20, cfg.dt,
                         plant=GpuPlant(ctx, h, psteps, sub), **kw)
        u = []
        for _ in range(steps):
            loop.step()
            u.append(loop.u0.cpu().numpy().copy())
        out = {}
        if adapt is not None:
            torch.cuda.synchronize()
            out = dict(count=loop.adapt_count, params_status=loop.params_status.cpu().numpy(),
                       ident_status=loop.ident_status.cpu().numpy(), in_force=np.asarray(ctx.get_params()))
        elif recorder is not None:
            # the plant's 21 are drawn +-10 % around the nominal row: a box that holds the draw
            icfg = ok.ident_default_config(h=cfg.dt, substeps=psteps * sub, lb_rel=0.5, ub_rel=0.5)
            res = [t.cpu().numpy() for t in recorder.identify(ctx, icfg)]
            torch.cuda.synchronize()
            Xh, Uh = recorder.X.cpu().numpy(), recorder.U.cpu().numpy()
            nominal = np.repeat(ctx.params.as_array()[None, ref.IDX], nk, axis=0)
            A, _, _, _ = ctx.ident_normal(Xh, Uh, nominal, None, icfg, wind=recorder.W.cpu().numpy())
            out = dict(res=res, A=A, windless=ctx.identify(Xh, Uh, None, icfg), icfg=icfg)
        return np.stack(u), loop.x0.cpu().numpy(), out
    finally:
        ctx.close()


def _dist(rows, plant, kp, live):
    """Scaled distance of each kite's 21 to the plant's over the excited parameters."""
    s = ref.scales(kp)
    return np.array([np.linalg.norm(((rows[b] - plant[b])[ref.IDX] / s)[live[b]]) for b in range(len(plant))])


def test_closed_loop_identification_under_wind(kp):
    nk, T = 8, 24
    plant = ok.perturb_params(kp, nk, 0.1, 71, fields=ok.IDENT_FIELDS)
    wind = np.random.default_rng(72).uniform(-1.5, 1.5, (nk, 3))
    rec = FlightRecorder(nk, T, "cuda", wind=True)
    u_rec, x_rec, out = _fly(nk, T + 1, plant, wind, rec)
    assert rec.full
    u_plain, x_plain, _ = _fly(nk, T + 1, plant, wind, None)
    np.testing.assert_array_equal(u_rec, u_plain)       # the recorder changes nothing
    np.testing.assert_array_equal(x_rec, x_plain)
    np.testing.assert_array_equal(rec.U.cpu().numpy(), np.transpose(u_rec[:T, :, :3], (1, 0, 2)))
    np.testing.assert_array_equal(rec.W.cpu().numpy(), np.repeat(wind[:, None], T, axis=1))
    rows, cost2, evals, status = out["res"]
    assert not (status & ok.IDENT_NAN).any()
    live = [np.diag(out["A"][b]) != 0.0 for b in range(nk)]          # parameters the loop excited
    nominal = np.repeat(kp[None], nk, axis=0)
    e_id, e_nom = _dist(rows, plant, kp, live), _dist(nominal, plant, kp, live)
    e_windless = _dist(out["windless"].params, plant, kp, live)      # for the record, not asserted
    for b in range(nk):
        assert rows[b, ref.IDX[~live[b]]].tobytes() == kp[ref.IDX[~live[b]]].tobytes()
        print(f"kite {b}: scaled distance to the plant's 21: nominal {e_nom[b]:.3e}, identified under the wind "
              f"{e_id[b]:.3e}, windless identification {e_windless[b]:.3e}; cost {cost2[b, 0]:.2e} -> "
              f"{cost2[b, 1]:.2e}, evals {evals[b]}, status {status[b]}")
    assert np.all(e_id < e_nom)
    assert np.all(cost2[:, 1] <= cost2[:, 0])

    # the same loop adapting: the identified rows become the controller's
    _, _, info = _fly(nk, T + 1, plant, wind, FlightRecorder(nk, T, "cuda", wind=True), adapt=out["icfg"])
    print(f"adapt: count {info['count']}, ident status {info['ident_status'].tolist()}, "
          f"params status {info['params_status'].tolist()}")
    assert info["count"] >= 1
    assert np.all(info["params_status"] == 0)
    e_ctl = _dist(info["in_force"], plant, kp, live)
    print(f"adapt: controller rows' distance {e_ctl.tolist()}")
    assert np.all(e_ctl < e_nom)


def test_ident_wind_estimate_logs_what_the_controller_was_given():
    """Plumbing only: row k of the recorder's wind log is the wind EKF's estimate
    as the controller received it in period k (non-finite -> 0, clamped to
    +-wind_max).  wind_max is small here so that the clamp is in play."""
    from bench import synthetic_x0
    nk, T, wmax = 4, 6, 0.05
    cfg = ok.default_config(N=20)
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    try:
        ctx.plant_set_wind(wind=np.random.default_rng(73).uniform(-1.5, 1.5, (nk, 3)))
        x_init = synthetic_x0(nk, 0, ctx)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        rec = FlightRecorder(nk, T, "cuda", wind=True)
        loop = FleetLoop(GpuStepper(ctx), torch.from_numpy(x_init).cuda(), 20, cfg.dt, wind_ekf=True,
                         covariances=ok.wind_ekf_default_covariances(), plant=GpuPlant(ctx, cfg.dt / 2, 2, 4),
                         wind_max=wmax, recorder=rec, ident_wind="estimate")
        # the first period filters nothing: what stands in the estimate is what the controller gets
        loop.xe[0, 13:16] = torch.tensor([math.nan, 100.0, -0.01], dtype=torch.float64)
        loop.xe[1, 13:16] = torch.tensor([math.inf, -100.0, 0.02], dtype=torch.float64)
        want = []
        for _ in range(T):
            loop.step()
            w = loop.xe[:, 13:16].cpu().numpy()         # the estimate in force during this period
            want.append(np.clip(np.where(np.isfinite(w), w, 0.0), -wmax, wmax))
        want = np.stack(want, axis=1)
        got = rec.W.cpu().numpy()
        print(f"estimates logged: {np.count_nonzero(np.abs(got) == wmax)} of {got.size} entries on the clamp")
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got[:2, 0], [[0.0, wmax, -0.01], [0.0, -wmax, 0.02]])
        assert not got[2:, 0].any()                     # the other estimates start at 0
    finally:
        ctx.close()
