"""GPU tests of the per-kite controller models (kite_nmpc_set_params[_device],
k_model_const, k_rk4_sens2<.., PERKITE>, k_prologue_pk / _cold_pk) and of the
loop that feeds them from the identification (FleetLoop(adapt=...)).

The reference of a heterogeneous batch is the oracle called kite by kite under
that kite's row (tests/perkite_cases.py).  Bars: the condensed QP data at 1e-11
(tests/test_wind.py, the same data), the RTI loops at the bars of
tests/test_gpu_parity.py for the homogeneous loop of the same horizon
(assert_cond_rti at N = 20, assert_ms_rti at N = 40); everything that is the
same arithmetic on the same values is compared bit for bit.

Shapes: B = 9 crosses the homogeneous kernel's 8-kite block; N = 20 is three
waves per kite in the per-kite sensitivity kernel, the last with 4 of 8 interval
groups; N = 40 is five full waves; B = 130 crosses the one-tangent kernel's
B <= 128 switch of the homogeneous path and two 64-lane blocks of
k_model_const."""
import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import FleetLoop, FlightRecorder, GpuPlant, GpuStepper
from oracle import ffi
from tests import perkite_cases as pc
from tests.test_gpu_parity import (COND_ENVELOPE, MS_ENVELOPE, assert_cond_rti, assert_ms_rti, gpu_to_oracle_perm,
                                   rel_per_kite)
from tests.test_wind import winds

pytestmark = pytest.mark.gpu

M, K = pc.M, pc.K
KEYS = ("u0", "traj", "ctrl", "status")


def make(B, Nh=20, **cfg):
    return ok.BatchNMPC(ok.load_properties(), ok.default_config(N=Nh, **cfg), B)


def fly(g, x, steps):
    """Closed loop on the GPU's own plan (the next measured state is node 1)."""
    out = []
    x = x.copy()
    for _ in range(steps):
        r = g.step(x)
        out.append(r)
        x = r["traj"][:, 1, :].copy()
    return out


def assert_same(a, b, kites=slice(None), kites_b=None):
    kb = kites if kites_b is None else kites_b
    for ra, rb in zip(a, b):
        for key in KEYS:
            np.testing.assert_array_equal(ra[key][kites], rb[key][kb], err_msg=key)


def nominal_rows(B):
    return np.repeat(ok.load_properties().as_array()[None], B, axis=0)


# ---- 1. identity ---------------------------------------------------------------
@pytest.mark.parametrize("Nh,B,windy", [(20, 9, False), (40, 3, False), (20, 9, True)])
def test_creation_rows_are_bitwise_the_homogeneous_step(Nh, B, windy):
    """All B rows equal to the creation row: the per-kite kernels compute what
    the homogeneous ones do, bit for bit -- cold step and 3 warm steps, and the
    condensed QP of the first and the last kite (N = 20)."""
    x = pc.states(B, 9200 + Nh, Nh)
    wd = winds(B, seed=3, vmax=0.5) if windy else None
    runs, qps = [], []
    for rows in (None, nominal_rows(B)):
        g = make(B, Nh)
        try:
            if wd is not None:
                g.set_wind(wd)
            if rows is not None:
                g.set_params(rows)
                np.testing.assert_array_equal(g.get_params(), rows)
            runs.append(fly(g, x, 4))
            if Nh == 20:
                qps.append([g.get_qp(b) for b in (0, B - 1)])
        finally:
            g.close()
    assert_same(runs[0], runs[1])
    for qa, qb in zip(*qps) if qps else ():
        for key in ("H", "h", "C", "cl", "cu"):
            np.testing.assert_array_equal(qa[key], qb[key], err_msg=key)


# ---- 2. parity against the per-kite oracle ---------------------------------------
def test_condensed_qp_vs_per_kite_oracle():
    """The condensed QP (the sensitivities and defects under each kite's own
    model, condensed) against ffi.build_qp(rows[b]) at 1e-11, on a cold step."""
    B, N = pc.B9, 20
    rows = pc.rows_for(B)
    cfgv = ffi.cfg_vector(dict(ffi.node_config(N=N), qp_form=0))
    x0 = pc.states(B, 9300)
    g = make(B, N, qp_kernel=2)
    try:
        g.set_params(rows)
        g.step(x0)
        perm = gpu_to_oracle_perm(N)
        for b in range(B):
            st, X, U, _ = ffi.prologue(rows[b], cfgv, N, M, x0[b], np.zeros((N + 1, 15)), np.zeros((N, 4)), warm=0)
            q = ffi.build_qp(rows[b], cfgv, N, M, X, U)
            gq = g.get_qp(b)
            Hg = np.zeros_like(q["H"]); Hg[np.ix_(perm, perm)] = gq["H"]
            hg = np.zeros_like(q["h"]); hg[perm] = gq["h"]
            Cg = np.zeros((N, 4 * N + 2)); Cg[:, perm] = gq["C"]
            e = (np.abs(Hg - q["H"]).max() / np.abs(q["H"]).max(),
                 np.abs(hg - q["h"]).max() / max(1.0, np.abs(q["h"]).max()),
                 np.abs(Cg - q["C"]).max() / max(1.0, np.abs(q["C"]).max()))
            print(f"kite {b}: H {e[0]:.2e} h {e[1]:.2e} C {e[2]:.2e}")
            assert max(e) < 1e-11, (b, e)
    finally:
        g.close()


def _check_step(g, r, ref, Nh, where):
    u0, Xo, Uo, diag, st = ref
    assert not np.any(r["status"] & 1) and not np.any(st & 1)
    np.testing.assert_array_equal(r["status"] & ~(2 | 32), st & ~(2 | 32))
    if Nh == 20:
        np.testing.assert_array_equal(r["status"] & 32, st & 32)
        worst = assert_cond_rti(r, u0, Xo, Uo, where)
    else:
        # as tests/test_wind.py: the step safeguard may decide differently only
        # where the two capped residuals straddle 1e-6 within a decade
        kg, ko = g.qp_stats()[0], diag[:, 5]
        flip = (np.minimum(kg, ko) < 1e-6) & (np.maximum(kg, ko) >= 1e-6) & (np.maximum(kg, ko) < 1e-5)
        same = (r["status"] & 32) == (st & 32)
        assert np.all(same | flip), (where, np.where(~same)[0], kg[~same], ko[~same])
        assert np.sum(~same) <= 1, np.where(~same)[0]
        e = np.maximum.reduce([rel_per_kite(r["u0"], u0), rel_per_kite(r["traj"], Xo),
                               rel_per_kite(r["ctrl"], Uo)])[same]
        assert_ms_rti(e, kg[same], ko[same], where)
        worst = float(e.max(initial=0.0))
    print(f"{where}: worst kite {worst:.2e}")


@pytest.mark.parametrize("Nh,B,steps,offset", [(20, pc.B9, 6, 9100), (40, 3, 3, 9140)])
def test_rti_loop_vs_per_kite_oracle(Nh, B, steps, offset):
    """Heterogeneous rows, closed loop on the oracle's plan (each GPU step starts
    from the oracle's solution): the bars of the homogeneous loop of the same
    horizon.  And the GPU's plan is as far from the NOMINAL-row oracle as the
    own-row oracle is (>= 1e3 bars, every kite): a build that ignored the rows
    cannot pass."""
    loop = pc.oracle_loop(Nh, B, steps, offset)
    nom = pc.oracle_nominal(Nh, B, steps, offset)
    bar = COND_ENVELOPE if Nh == 20 else MS_ENVELOPE
    g = make(B, Nh)
    try:
        g.set_params(pc.rows_for(B))
        for step, (x, u0, Xo, Uo, diag, st) in enumerate(loop):
            if step > 0:
                g.set_solution(loop[step - 1][2], loop[step - 1][3])
            r = g.step(x)
            _check_step(g, r, (u0, Xo, Uo, diag, st), Nh, (Nh, step))
            if step in nom:
                gap = pc.plan_gap(r["u0"], r["traj"], r["ctrl"], nom[step])
                assert np.all(gap >= pc.GAP * bar), (step, gap)
    finally:
        g.close()


def _oracle_run(rows, cv, Nh, x, steps, wind=None, drift=False):
    B = x.shape[0]
    X = np.zeros((B, Nh + 1, 15)); U = np.zeros((B, Nh, 4))
    out = []
    for step in range(steps):
        u0, diag, st = pc.oracle_step(rows, cv, Nh, x, X, U, warm=int(step > 0), wind=wind)
        out.append((x.copy(), u0, X.copy(), U.copy(), diag, st))
        x = X[:, 1, :].copy()
        if drift:       # as test_gpu_parity.test_delay_compensation_vs_oracle: the compensation has work to do
            x[:, :3] *= 1.002
            x[:, 13:] = 0.0
    return out


@pytest.mark.parametrize("case", ["delay", "wind"])
def test_rti_loop_with_delay_and_with_wind_vs_per_kite_oracle(case):
    """The prologue's delay compensation (k_prologue_pk on every step) and the
    WIND instances under per-kite rows, 4 closed-loop steps of 9 kites."""
    B, N, steps = pc.B9, 20, 4
    rows = pc.rows_for(B)
    c = ffi.node_config()
    cfg, wd = {}, None
    if case == "delay":
        c["delay"], c["delay_steps"] = 0.1, 16
        cfg = dict(delay=0.1, delay_steps=16)
    else:
        wd = winds(B, seed=21)
    cv = ffi.cfg_vector(c)
    loop = _oracle_run(rows, cv, N, pc.states(B, 9400), steps, wind=wd, drift=case == "delay")
    g = make(B, N, **cfg)
    try:
        g.set_params(rows)
        if wd is not None:
            g.set_wind(wd)
        for step, (x, u0, Xo, Uo, diag, st) in enumerate(loop):
            if step > 0:
                g.set_solution(loop[step - 1][2], loop[step - 1][3])
            r = g.step(x)
            _check_step(g, r, (u0, Xo, Uo, diag, st), N, (case, step))
    finally:
        g.close()


# ---- 3. batch invariance -----------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """B = 130 heterogeneous kites, one (row, state) repeated at 0, 7, 8, 129."""
    B, pos = 130, (0, 7, 8, 129)
    rows = pc.rows_for(B)
    x = pc.states(B, 9500)
    for p in pos:
        rows[p] = rows[40]
        x[p] = x[40]
    g = make(B)
    try:
        g.set_params(rows)
        run = fly(g, x, 3)
    finally:
        g.close()
    return dict(B=B, pos=pos, rows=rows, x=x, run=run)


def test_a_kite_does_not_depend_on_the_batch_around_it(big):
    """Alone (B = 1, the one-model form: kernel-argument model, k_rk4_sens1) ==
    inside B = 130 at positions 0, 7, 8, 129 (the table, the one-kite-per-wave
    kernel), bitwise over a cold and two warm steps."""
    g = make(1)
    try:
        g.set_params(big["rows"][40])
        np.testing.assert_array_equal(g.get_params()[0], big["rows"][40])
        alone = fly(g, big["x"][40:41], 3)
    finally:
        g.close()
    for p in big["pos"] + (40,):
        assert_same(alone, big["run"], slice(0, 1), slice(p, p + 1))


def test_permuting_rows_and_states_permutes_the_outputs(big):
    perm = np.random.default_rng(5).permutation(big["B"])
    g = make(big["B"])
    try:
        g.set_params(big["rows"][perm])
        run = fly(g, big["x"][perm], 3)
    finally:
        g.close()
    assert_same(run, big["run"], slice(None), perm)


# ---- 4. setters ------------------------------------------------------------------------
def test_host_and_device_setters_agree_and_switch_back():
    B = pc.B9
    rows = pc.rows_for(B)
    x = pc.states(B, 9600)
    g0 = make(B)
    try:
        base = fly(g0, x, 3)
    finally:
        g0.close()
    gh, gd = make(B), make(B)
    try:
        gh.set_params(rows)
        d_rows = torch.from_numpy(rows.copy()).cuda()
        d_st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
        gd.set_params_device(d_rows.data_ptr(), B, d_st.data_ptr())
        np.testing.assert_array_equal(gh.get_params(), rows)
        np.testing.assert_array_equal(gd.get_params(), rows)
        assert not d_st.cpu().numpy().any()                 # written, not OR-ed
        rh, rd = fly(gh, x, 3), fly(gd, x, 3)
        assert_same(rh, rd)
        assert any(not np.array_equal(a["traj"], b["traj"]) for a, b in zip(rh, base))   # the rows are live
        # back to the creation model, by NULL and by the one-model form with the creation row
        gh.set_params(None)
        gh.reset()
        np.testing.assert_array_equal(gh.get_params(), nominal_rows(B))
        assert_same(fly(gh, x, 3), base)
        gd.set_params(ok.load_properties())
        gd.reset()
        np.testing.assert_array_equal(gd.get_params(), nominal_rows(B))
        assert_same(fly(gd, x, 3), base)
    finally:
        gh.close(); gd.close()


def test_refreshing_the_rows_between_steps():
    """New rows between two steps through the device setter (the captured step
    graph stays: it reads the table when it runs) == a fresh context set once
    to those rows and warm-started from the same solution."""
    B = pc.B9
    rows_a, rows_b = pc.rows_for(B), pc.rows_for(B, seed=pc.SEED + 1)
    x = pc.states(B, 9700)
    g, f = make(B), make(B)
    try:
        d_a = torch.from_numpy(rows_a.copy()).cuda()
        d_b = torch.from_numpy(rows_b.copy()).cuda()
        g.set_params_device(d_a.data_ptr(), B)
        run = fly(g, x, 2)
        sol = g.get_solution()
        x2 = run[-1]["traj"][:, 1, :].copy()
        g.set_params_device(d_b.data_ptr(), B)
        r1 = g.step(x2)
        f.set_params(rows_b)
        f.set_solution(*sol)
        r2 = f.step(x2)
        assert_same([r1], [r2])
        np.testing.assert_array_equal(g.get_params(), rows_b)
    finally:
        g.close(); f.close()


# ---- 5. containment ------------------------------------------------------------------
def test_a_row_that_is_no_model_is_contained():
    B = pc.B9
    fld = nmpc._PARAM_FIELDS.index
    rows_a, rows_b = pc.rows_for(B), pc.rows_for(B, seed=pc.SEED + 1)
    bad = rows_b.copy()
    bad[1, fld("Cma")] = np.nan
    bad[4, fld("mass")] = 0.0
    bad[6, [fld("Ixx"), fld("Izz"), fld("Ixz")]] = (1.0, 4.0, 2.0)       # Ixx Izz - Ixz^2 == 0
    expect = rows_b.copy()
    expect[[1, 4, 6]] = rows_a[[1, 4, 6]]
    x = pc.states(B, 9800)
    g, c = make(B), make(B)
    try:
        st = torch.zeros((B,), dtype=torch.int32, device="cuda")
        d = torch.from_numpy(rows_a.copy()).cuda()
        g.set_params_device(d.data_ptr(), B, st.data_ptr())
        assert not st.cpu().numpy().any()
        d.copy_(torch.from_numpy(bad))
        g.set_params_device(d.data_ptr(), B, st.data_ptr())
        want = np.zeros(B, dtype=np.int32); want[[1, 4, 6]] = nmpc.PARAMS_REJECTED
        np.testing.assert_array_equal(st.cpu().numpy(), want)
        np.testing.assert_array_equal(g.get_params(), expect)
        c.set_params(expect)
        run = fly(g, x, 3)
        assert_same(run, fly(c, x, 3))
        # the host setter refuses the whole call and changes nothing
        for rows in (bad, bad[[0, 1, 2]], rows_b[:4]):
            with pytest.raises(ok.KiteNmpcError) as e:
                g.set_params(rows)
            assert e.value.code == nmpc.KITE_EINVAL
        with pytest.raises(ok.KiteNmpcError) as e:
            g.set_params_device(d.data_ptr(), 4)
        assert e.value.code == nmpc.KITE_EINVAL
        with pytest.raises(ok.KiteNmpcError) as e:
            g.set_params_device(0, B)
        assert e.value.code == nmpc.KITE_EINVAL
        np.testing.assert_array_equal(g.get_params(), expect)
        g.reset()
        assert_same(fly(g, x, 3), run)
    finally:
        g.close(); c.close()


def test_a_first_call_rejection_keeps_the_creation_model():
    B = pc.B9
    rows = pc.rows_for(B)
    rows[3, nmpc._PARAM_FIELDS.index("mass")] = -1.0
    g = make(B)
    try:
        st = torch.zeros((B,), dtype=torch.int32, device="cuda")
        d = torch.from_numpy(rows.copy()).cuda()
        g.set_params_device(d.data_ptr(), B, st.data_ptr())
        assert st.cpu().numpy().tolist() == [0, 0, 0, nmpc.PARAMS_REJECTED] + [0] * (B - 4)
        got = g.get_params()
        np.testing.assert_array_equal(got[3], ok.load_properties().as_array())
        np.testing.assert_array_equal(np.delete(got, 3, 0), np.delete(rows, 3, 0))
    finally:
        g.close()


def test_fp32_sensitivities_hold_one_model():
    B = 4
    rows = pc.rows_for(B)
    g = make(B, sens_fp32=1)
    try:
        with pytest.raises(ok.KiteNmpcError) as e:
            g.set_params(rows)
        assert e.value.code == nmpc.KITE_ESTATE
        d = torch.from_numpy(rows.copy()).cuda()
        with pytest.raises(ok.KiteNmpcError) as e:
            g.set_params_device(d.data_ptr(), B)
        assert e.value.code == nmpc.KITE_ESTATE
        g.set_params(rows[0])           # one model for all: the kernel-argument path
        np.testing.assert_array_equal(g.get_params(), np.repeat(rows[:1], B, axis=0))
    finally:
        g.close()


# ---- 6. closed loop: plant -> recorder -> identification -> controller ---------------------
def _closed_loop(nk, T, steps, plant_rows, adapt, informed):
    from bench import synthetic_x0
    cfg = ok.default_config(N=20)
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    try:
        ctx.plant_set_params(plant_rows)
        if informed:
            ctx.set_params(plant_rows)
        x_init = synthetic_x0(nk, 0, ctx)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        kw = dict(recorder=FlightRecorder(nk, T, "cuda"), adapt=adapt) if adapt is not None else {}
        loop = FleetLoop(GpuStepper(ctx), torch.from_numpy(x_init).cuda(), 20, cfg.dt,
                         plant=GpuPlant(ctx, cfg.dt, 1, 2), **kw)
        rows0 = loop.model_rows.clone() if adapt is not None else None
        err, log = [], []
        for _ in range(steps):      # nothing here waits for the device
            xk = loop.x0[:, :13].clone()
            loop.step()
            err.append((loop.traj[:, 1, :13] - loop.x0[:, :13]).abs().amax(dim=1))
            log.append((xk, loop.u0.clone(), loop.x0[:, :13].clone()))
        err = torch.stack(err).cpu().numpy()            # (steps, nk)
        info = None
        if adapt is not None:
            info = dict(count=loop.adapt_count, ident=loop.ident_status.cpu().numpy(),
                        params=loop.params_status.cpu().numpy(), rows=loop.model_rows.cpu().numpy(),
                        rows0=rows0.cpu().numpy(), in_force=ctx.get_params(),
                        log=[tuple(t.cpu().numpy() for t in rec) for rec in log])

            def model_error(rows, lo, hi):
                """Per kite, the median over steps lo..hi-1 of |x+ predicted by the
                model `rows` from the logged (x, u0) - the x the plant produced|_inf:
                the controller's RK4 arithmetic (h = dt, 2 substeps), no linearisation."""
                ctx.plant_set_params(rows)
                e = [np.abs(ctx.plant_step(x, u, 0.0, cfg.dt, 1, 2)[0] - xn).max(1) for x, u, xn in info["log"][lo:hi]]
                return np.median(np.stack(e), axis=0)
            info["model_error"] = model_error
            info["nominal"] = model_error(ctx.params, 5, T)
            info["adapted"] = model_error(info["in_force"], T, steps)
            info["true"] = model_error(plant_rows, T, steps)
        return err, info
    finally:
        ctx.close()


def test_closed_loop_adaptation():
    """8 kites fly a plant whose 21 aerodynamic coefficients are +-10 % off the
    controller's; the plant integrates with the controller's own RK4 arithmetic
    (h = dt, 2 substeps), so the parameters are the only mismatch.  After 25
    periods the loop identifies them and hands them to the controller on the
    stream.  Per kite, the one-step prediction error |traj[:, 1, :13] - x
    measured at the next step|_inf, median over steps 5..24 (before) and over
    the 10 steps after the adaptation.

    Bar (derived, not measured): f is at most quadratic in the 21, so the
    prediction error is essentially linear in the parameter error, which falls
    from 0.25..0.31 to <= 3.3e-11 in scaled distance (the identification's
    recorded closed-loop result): a factor 1e-10, asserted as 1e-6.  Where the
    absolute rounding floor limits the ratio, 100 x the error of the informed
    loop (the controller given the plant's true rows from step 0)."""
    nk, T, after = 8, 25, 10
    plant = ok.perturb_params(ok.load_properties(), nk, 0.1, 71, fields=ok.IDENT_FIELDS)
    cfg = ok.default_config(N=20)
    icfg = ok.ident_default_config(h=cfg.dt, substeps=2, lb_rel=0.5, ub_rel=0.5)
    err, info = _closed_loop(nk, T, T + after, plant, icfg, False)
    err_inf, _ = _closed_loop(nk, T, T + after, plant, None, True)
    before = np.median(err[5:T], axis=0)
    aft = np.median(err[T:T + after], axis=0)
    floor = np.median(err_inf[T:T + after], axis=0)
    for b in range(nk):
        branch = "1e-6 x before" if 1e-6 * before[b] >= 100 * floor[b] else "100 x informed"
        print(f"kite {b}: before {before[b]:.3e} after {aft[b]:.3e} ratio {aft[b] / before[b]:.2e} "
              f"informed {floor[b]:.3e} (informed / before {floor[b] / before[b]:.2e}) bar: {branch} "
              f"ident status {info['ident'][b]} params status {info['params'][b]}")
    assert info["count"] == 1
    assert np.all(info["ident"] & nmpc.IDENT_CONVERGED) and not np.any(info["ident"] & nmpc.IDENT_NAN)
    assert not info["params"].any()
    assert np.all(np.any(info["rows"] != info["rows0"], axis=1))          # all 8 accepted
    np.testing.assert_array_equal(info["in_force"], info["rows"])
    assert np.all(before > 1e-6)                                            # there was a mismatch to remove
    assert np.all(aft <= np.maximum(1e-6 * before, 100 * floor)), (aft, before, floor)
    # The plan's node 1 is a LINEARISED prediction (one Newton step of the RTI),
    # and its linearisation error -- 0.07..0.14 here even in the informed loop --
    # hides the parameter error: the assertion above takes its second branch for
    # every kite and could not fail.  The bar's derivation is about the MODEL,
    # so it is also asserted there: the one-step prediction of the rows in force
    # in the controller (read back through kite_nmpc_get_params), evaluated with
    # the controller's RK4 arithmetic on the logged (x, u0), against the state
    # the plant produced -- nominal rows before, adapted rows after, and the
    # plant's true rows as the rounding floor (the same arithmetic: zero).
    nomi, adap, true = info["nominal"], info["adapted"], info["true"]
    for b in range(nk):
        print(f"kite {b}: model one-step error: nominal rows {nomi[b]:.3e}, adapted rows {adap[b]:.3e} "
              f"(ratio {adap[b] / nomi[b]:.2e}), true rows {true[b]:.3e}")
    assert np.all(nomi > 1e-6)
    assert np.all(adap <= np.maximum(1e-6 * nomi, 100 * true)), (adap, nomi, true)
