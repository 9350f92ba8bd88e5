"""GPU tests of the per-kite estimator models: k_ekf_pk and k_ekf_wind_pk fed
from the controller's table (kite_nmpc_set_estimator_model), and
``FleetLoop(estimator_model="controller")``.

The reference of a heterogeneous batch is the CPU filter called kite by kite
under that kite's row (tests/ekf_perkite_cases.py; checked on the CPU in
test_ekf_perkite_ref.py).  Bars: test_ekf.py's and test_wind_ekf.py's -- x13
rtol 1e-12, the 13-state block of P rtol 1e-11 (atol 1e-13), the wind entries
10 x the reference's two-run envelope, not below 1e-11, computed from the
reference alone.  Everything that is the same arithmetic on the same values is
compared bit for bit.

Shapes: in the homogeneous kernels B = 4 is one full block of four kites, 5 a
ragged block, 130 is 33 blocks, and positions 0, 3, 4 and 129 are the first and
last kite of a full block, the first of the next and the only kite of the
ragged one; the per-kite kernels run one 16-thread block per kite, so the same
shapes are 4, 5 and 130 blocks.  k_ekf has no substep loop: its "substeps 5" is
five calls of dt / 5 with the update on the last, as FleetLoop drives it.

Measured on an MI355X, worst over the parity cases in units of the bar: k_ekf_pk
x 0.002 and P 0.003; k_ekf_wind_pk x13 0.040, the 13-state block of P 0.077, the
wind entries 6.1e-14 absolute against the 1e-11 floor (reference envelope
<= 6.3e-14); the smallest distance of the GPU's output to the nominal row's
reference 5.9e9 bars.  Open loop: see test_open_loop_gpu_meets_reference.
"""
import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import FleetLoop, GpuPlant, GpuStepper
from tests import ekf_perkite_cases as ec
from tests import perkite_cases as pc

pytestmark = pytest.mark.gpu

DT = ec.DT
CASES = [(s, up) for s in (1, 5) for up in (False, True)]


def make(B, Nh=20):
    return ok.BatchNMPC(ok.load_properties(), ok.default_config(N=Nh), B)


def creation_rows(B):
    return np.repeat(ok.load_properties().as_array()[None], B, axis=0)


@pytest.fixture(scope="module")
def pool():
    """Contexts of B kites with rows_for(B) in the controller (host setter) and
    the estimators on the controller's models; shared, so tests leave them so."""
    made = {}

    def get(B):
        if B not in made:
            g = make(B)
            g.set_params(ec.rows_for(B))
            g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
            made[B] = g
        return made[B]
    yield get
    for g in made.values():
        g.close()


def sl(inputs, B, perm=None):
    """The first B kites (or the kites perm) of the per-kite inputs; W, V whole."""
    idx = slice(0, B) if perm is None else perm
    return tuple(a[idx] if i < 4 else a for i, a in enumerate(inputs))


def run_ekf(g, inp, substeps, update):
    x, u, P, z, W, V = inp
    for s in range(substeps):
        x, P = g.ekf_step(x, u, P, DT / substeps, z if (update and s == substeps - 1) else None, W, V)
    return x, P


def run_wind(g, inp, substeps, update):
    x16, u, P, z, W, V = inp
    return g.wind_ekf_step(x16, u, P, DT, substeps, z if update else None, W, V)


def everything(g, B, perm=None):
    """Both filters over CASES on the first B kites: {(filter, substeps, update): arrays}."""
    out = {}
    for s, up in CASES:
        out["ekf", s, up] = run_ekf(g, sl(ec.ekf_inputs(), B, perm), s, up)
        out["wind", s, up] = run_wind(g, sl(ec.wind_inputs(), B, perm), s, up)
    return out


def assert_same(a, b, kites=slice(None), kites_b=None):
    kb = kites if kites_b is None else kites_b
    assert a.keys() == b.keys()
    for key in a:
        for va, vb in zip(a[key], b[key]):
            np.testing.assert_array_equal(va[kites], vb[kb], err_msg=str(key))


def check_ekf(xg, Pg, xr, Pr, where):
    print(f"{where}: x13 worst error / bar {ec.worst(xg, xr, ec.X_RTOL):.3f}, P {ec.worst(Pg, Pr, ec.P_RTOL):.3f}")
    np.testing.assert_allclose(xg, xr, rtol=ec.X_RTOL, atol=ec.ATOL)
    np.testing.assert_allclose(Pg, Pr, rtol=ec.P_RTOL, atol=ec.ATOL)


def check_wind(xg, Pg, a, b, where):
    env, bar = ec.wind_bar(a, b)
    err = float(np.abs(ec.wind_entries(xg, Pg) - ec.wind_entries(a[0], a[1])).max())
    print(f"{where}: x13 worst error / bar {ec.worst(xg[:, :13], a[0][:, :13], ec.X_RTOL):.3f}, P 13-state block "
          f"{ec.worst(Pg[:, :13, :13], a[1][:, :13, :13], ec.P_RTOL):.3f}, wind entries {err:.3e} "
          f"(reference envelope {env:.3e}, bar {bar:.3e})")
    np.testing.assert_allclose(xg[:, :13], a[0][:, :13], rtol=ec.X_RTOL, atol=ec.ATOL)
    np.testing.assert_allclose(Pg[:, :13, :13], a[1][:, :13, :13], rtol=ec.P_RTOL, atol=ec.ATOL)
    assert err <= bar


# ---- 1. identity ---------------------------------------------------------------
@pytest.mark.parametrize("B", [5, 130])
def test_creation_rows_are_bitwise_the_creation_model(B):
    """Mode 1 with B rows equal to the creation row gives the mode-0 outputs bit
    for bit (x, P, status; both filters, substeps 1 and 5, with and without z);
    mode 0 gives them whatever rows the controller holds."""
    g = make(B)
    try:
        assert g.estimator_model == ok.EST_MODEL_CREATION
        base = everything(g, B)
        g.set_params(ec.rows_for(B))                     # heterogeneous rows, estimators on mode 0
        assert_same(everything(g, B), base)
        g.set_params(creation_rows(B))
        g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        assert_same(everything(g, B), base)
        assert not any(v[2].any() for k, v in base.items() if k[0] == "wind")
    finally:
        g.close()


# ---- 2. parity against the per-kite reference ------------------------------------
@pytest.mark.parametrize("substeps,update", CASES)
@pytest.mark.parametrize("B", [4, 5, 130])
def test_filters_vs_per_kite_reference(pool, B, substeps, update):
    g = pool(B)
    where = f"B {B} substeps {substeps} update {update}"
    xg, Pg = run_ekf(g, sl(ec.ekf_inputs(), B), substeps, update)
    xr, Pr = ec.ekf_reference(B, substeps, update)
    check_ekf(xg, Pg, xr, Pr, "k_ekf " + where)
    xw, Pw, st = run_wind(g, sl(ec.wind_inputs(), B), substeps, update)
    assert not st.any()
    a = ec.wind_reference(B, substeps, update)
    check_wind(xw, Pw, a, ec.wind_reference(B, substeps, update, alt=True), "k_ekf_wind " + where)
    # a build that ignored the table would sit on the nominal row's reference:
    # the GPU is as far from that as the per-kite reference is (test_ekf_perkite_ref.py)
    xn, Pn = ec.ekf_reference(B, substeps, update, own_rows=False)
    wn = ec.wind_reference(B, substeps, update, own_rows=False)
    gaps = (ec.worst_per_kite(xg, xn, ec.X_RTOL), ec.worst_per_kite(Pg, Pn, ec.P_RTOL),
            ec.worst_per_kite(xw[:, :13], wn[0][:, :13], ec.X_RTOL))
    print("smallest distance to the nominal row's reference, in bars:", " ".join(f"{v.min():.1e}" for v in gaps))
    assert all(np.all(v >= ec.GAP) for v in gaps)


# ---- 3. batch invariance --------------------------------------------------------
def test_a_kite_alone_equals_the_kite_in_the_batch(pool):
    """B = 1 with the kite's row in the one-model form runs the homogeneous
    kernels; the same kite at positions 0, 3, 4 and 129 of B = 130 runs the
    per-kite ones: bit for bit the same."""
    B = ec.BMAX
    rows = ec.rows_for(B)
    big = everything(pool(B), B)
    one = make(1)
    try:
        one.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        for p in (0, 3, 4, 129):
            one.set_params(rows[p])
            assert_same(everything(one, 1, perm=np.array([p])), big, kites=slice(None), kites_b=slice(p, p + 1))
    finally:
        one.close()


def test_permuted_rows_and_inputs_permute_the_outputs(pool):
    B = ec.BMAX
    perm = np.random.default_rng(11).permutation(B)
    big = everything(pool(B), B)
    g = make(B)
    try:
        g.set_params(ec.rows_for(B)[perm])
        g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        assert_same(everything(g, B, perm=perm), big, kites=slice(None), kites_b=perm)
    finally:
        g.close()


# ---- 4. setters and ordering ------------------------------------------------------
def test_host_rows_equal_device_rows(pool):
    B = 5
    g = make(B)
    try:
        g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        d = torch.from_numpy(ec.rows_for(B).copy()).cuda()
        g.set_params_device(d.data_ptr(), B)
        assert_same(everything(g, B), everything(pool(B), B))
    finally:
        g.close()


def _device_inputs(B):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return [dev(a) for a in sl(ec.wind_inputs(), B)], [dev(a) for a in sl(ec.ekf_inputs(), B)]


def test_rows_set_on_the_stream_reach_the_next_filter_step():
    """set_params_device(rows2) and then the filters, on one stream with no
    synchronisation in between, equal a fresh context set once with rows2."""
    B = 5
    rows_a, rows_b = ec.rows_for(B), ec.rows_for(B, seed=pc.SEED + 1)
    g, f = make(B), make(B)
    try:
        g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        g.set_stream(torch.cuda.current_stream().cuda_stream)
        d_a, d_b = torch.from_numpy(rows_a.copy()).cuda(), torch.from_numpy(rows_b.copy()).cuda()
        (wx, wu, wP, wz, wW, wV), (ex, eu, eP, ez, eW, eV) = _device_inputs(B)
        wx0, wP0 = wx.clone(), wP.clone()
        st = torch.zeros((B,), dtype=torch.int32, device="cuda")
        g.set_params_device(d_a.data_ptr(), B)
        g.wind_ekf_step_device(B, DT, 5, wx0.data_ptr(), wu.data_ptr(), wP0.data_ptr(), wz.data_ptr(), wW.data_ptr(),
                               wV.data_ptr(), st.data_ptr())           # a step under rows_a keeps the stream busy
        g.set_params_device(d_b.data_ptr(), B)
        g.wind_ekf_step_device(B, DT, 5, wx.data_ptr(), wu.data_ptr(), wP.data_ptr(), wz.data_ptr(), wW.data_ptr(),
                               wV.data_ptr(), st.data_ptr())
        g.ekf_step_device(B, DT, ex.data_ptr(), eu.data_ptr(), eP.data_ptr(), ez.data_ptr(), eW.data_ptr(),
                          eV.data_ptr())
        torch.cuda.synchronize()
        f.set_params(rows_b)
        f.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        xw, Pw, sw = run_wind(f, sl(ec.wind_inputs(), B), 5, True)
        xe, Pe = run_ekf(f, sl(ec.ekf_inputs(), B), 1, True)
        np.testing.assert_array_equal(wx.cpu().numpy(), xw)
        np.testing.assert_array_equal(wP.cpu().numpy(), Pw)
        np.testing.assert_array_equal(st.cpu().numpy(), sw)
        np.testing.assert_array_equal(ex.cpu().numpy(), xe)
        np.testing.assert_array_equal(eP.cpu().numpy(), Pe)
        # and the step before it ran under rows_a
        assert not np.array_equal(wx0.cpu().numpy(), xw)
    finally:
        g.use_own_stream()
        g.close(); f.close()


def test_a_rejected_row_keeps_the_kites_previous_model_in_the_filters():
    B = 5
    fld = nmpc._PARAM_FIELDS.index
    rows_a, rows_b = ec.rows_for(B), ec.rows_for(B, seed=pc.SEED + 1)
    bad = rows_b.copy()
    bad[1, fld("Cma")] = np.nan
    bad[3, fld("mass")] = 0.0
    expect = rows_b.copy(); expect[[1, 3]] = rows_a[[1, 3]]
    g, c, clean = make(B), make(B), make(B)
    try:
        st = torch.zeros((B,), dtype=torch.int32, device="cuda")
        d = torch.from_numpy(rows_a.copy()).cuda()
        g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        g.set_params_device(d.data_ptr(), B, st.data_ptr())
        g.synchronize()
        d.copy_(torch.from_numpy(bad))
        torch.cuda.synchronize()
        g.set_params_device(d.data_ptr(), B, st.data_ptr())
        got = everything(g, B)
        assert st.cpu().numpy().tolist() == [0, nmpc.PARAMS_REJECTED, 0, nmpc.PARAMS_REJECTED, 0]
        for ctx, rows in ((c, expect), (clean, rows_b)):
            ctx.set_params(rows)
            ctx.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        assert_same(got, everything(c, B))                       # kites 1 and 3 filter with the rows they kept
        assert_same(got, everything(clean, B), kites=[0, 2, 4])  # the others are the clean run
    finally:
        g.close(); c.close(); clean.close()


@pytest.mark.parametrize("count", [1, 4, 5, 7])
def test_one_model_form_vs_reference_at_every_count(count):
    """One perturbed row for every kite (the kernel-argument path): the
    homogeneous kernels under that row, at counts below, at and above B."""
    B = 5
    row = ec.rows_for(B)[2]
    g = make(B)
    try:
        g.set_params(row)
        g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        for s, up in ((1, False), (5, True)):
            ei, wi = sl(ec.ekf_inputs(), count), sl(ec.wind_inputs(), count)
            xg, Pg = run_ekf(g, ei, s, up)
            xr, Pr = ec.ekf_ref(row, ei[0], ei[1], ei[2], DT, s, ei[3] if up else None, ei[4], ei[5])
            check_ekf(xg, Pg, xr, Pr, f"k_ekf count {count} substeps {s}")
            xw, Pw, st = run_wind(g, wi, s, up)
            assert not st.any()
            a = ec.wind_ref(row, wi[0], wi[1], wi[2], DT, s, wi[3] if up else None, wi[4], wi[5])
            b = ec.wind_ref(row, wi[0], wi[1], wi[2], DT, s, wi[3] if up else None, wi[4], wi[5],
                            ec.ref.FD_STEPS_ALT)
            check_wind(xw, Pw, a, b, f"k_ekf_wind count {count} substeps {s}")
    finally:
        g.close()


# ---- 5. refusals -----------------------------------------------------------------
def test_refusals(pool):
    B = 5
    g = pool(B)
    # a table in force and count != B: KITE_EINVAL, nothing launched
    (wx, wu, wP, wz, wW, wV), (ex, eu, eP, ez, eW, eV) = _device_inputs(7)
    keep = [t.clone() for t in (wx, wP, ex, eP)]
    st = torch.full((7,), 9, dtype=torch.int32, device="cuda")
    for count in (4, 7):
        with pytest.raises(ok.KiteNmpcError) as e:
            g.wind_ekf_step_device(count, DT, 5, wx.data_ptr(), wu.data_ptr(), wP.data_ptr(), wz.data_ptr(),
                                   wW.data_ptr(), wV.data_ptr(), st.data_ptr())
        assert e.value.code == nmpc.KITE_EINVAL
        with pytest.raises(ok.KiteNmpcError) as e:
            g.ekf_step_device(count, DT, ex.data_ptr(), eu.data_ptr(), eP.data_ptr(), ez.data_ptr(), eW.data_ptr(),
                              eV.data_ptr())
        assert e.value.code == nmpc.KITE_EINVAL
        with pytest.raises(ok.KiteNmpcError) as e:
            run_wind(g, sl(ec.wind_inputs(), count), 1, True)
        assert e.value.code == nmpc.KITE_EINVAL
        with pytest.raises(ok.KiteNmpcError) as e:
            run_ekf(g, sl(ec.ekf_inputs(), count), 1, True)
        assert e.value.code == nmpc.KITE_EINVAL
    g.synchronize(); torch.cuda.synchronize()
    for t, k in zip((wx, wP, ex, eP), keep):
        assert torch.equal(t, k)
    assert st.cpu().numpy().tolist() == [9] * 7
    # modes
    for mode in (-1, 2, 7):
        with pytest.raises(ok.KiteNmpcError) as e:
            g.set_estimator_model(mode)
        assert e.value.code == nmpc.KITE_EINVAL
        assert g.estimator_model == ok.EST_MODEL_CONTROLLER
    g.set_estimator_model(ok.EST_MODEL_CREATION)
    assert g.estimator_model == ok.EST_MODEL_CREATION
    # mode 0 takes any count again
    assert not run_wind(g, sl(ec.wind_inputs(), 7), 1, True)[2].any()
    g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
    assert g.estimator_model == ok.EST_MODEL_CONTROLLER


# ---- 6. containment under per-kite rows ---------------------------------------------
def test_nan_kite_is_left_alone_and_flagged(pool):
    B = 5
    g = pool(B)
    x16, u, P, z, W, V = sl(ec.wind_inputs(), B)
    clean = g.wind_ekf_step(x16, u, P, DT, 5, z, W, V)
    bad = x16.copy(); bad[2, 4] = np.nan
    xg, Pg, st = g.wind_ekf_step(bad, u, P, DT, 5, z, W, V)
    assert st.tolist() == [0, 0, ok.EKF_NAN, 0, 0]
    np.testing.assert_array_equal(xg[2], bad[2])            # NaN in the same place, the rest untouched
    np.testing.assert_array_equal(Pg[2], P[2])
    for k in (0, 1, 3, 4):                                   # 0, 1, 3: the other kites of its block
        np.testing.assert_array_equal(xg[k], clean[0][k])
        np.testing.assert_array_equal(Pg[k], clean[1][k])


# ---- 7. open loop -------------------------------------------------------------------
@pytest.fixture(scope="module")
def open_loop_gpu():
    """The open-loop run of ekf_perkite_cases (truth under rows_for(8)) through
    k_ekf_wind_pk, the controller's rows equal to the truth's."""
    tr = ec.open_loop_truth()
    W, V, _ = ok.wind_ekf_default_covariances()
    g = make(ec.OL_B)
    try:
        g.set_params(tr["rows"])
        g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        xe, P = ec.open_loop_start()
        flags = 0
        for t in range(ec.OL_T):
            xe, P, st = g.wind_ekf_step(xe, tr["u"], P, ec.OL_DT, 1, tr["z"][t], W, V)
            flags |= int(np.bitwise_or.reduce(st))
    finally:
        g.close()
    return xe, P, flags


def test_open_loop_wind_convergence(open_loop_gpu):
    xe, P, flags = open_loop_gpu
    ratio = ec.wind_error_ratio(xe)
    print("gpu final / initial wind error", np.round(ratio, 3))
    assert flags == 0
    assert np.all(ratio <= 0.25), ratio


def test_open_loop_gpu_meets_reference(open_loop_gpu):
    """After the 40 periods the GPU meets the per-kite reference.  Each bar is
    the larger of the module's fixed bar and 10 x the reference's own two-run
    envelope on those entries (the fixed P bar alone is not supported at the
    end of this run: the reference's two runs differ by 1.2 x it on the
    13-state block); computed from the reference alone.

    Measured on an MI355X: reference envelope x13 1.3e-14 (0.06 fixed bars), P
    block 5.9e-13 (1.22 fixed bars), wind entries 7.7e-13; GPU error x13 1.9e-14
    (0.084 of its bar), P block 4.2e-13 (0.071), wind entries 1.7e-12 (bar
    1e-11)."""
    xg, Pg, _ = open_loop_gpu
    a, b = ec.open_loop_reference(True), ec.open_loop_reference(True, alt=True)
    env_x = float(np.abs(a[0][:, :13] - b[0][:, :13]).max())
    env_P = float(np.abs(a[1][:, :13, :13] - b[1][:, :13, :13]).max())
    env_w, bar_w = ec.wind_bar(a, b)
    bar_x = np.maximum(ec.ATOL + ec.X_RTOL * np.abs(a[0][:, :13]), 10.0 * env_x)
    bar_P = np.maximum(ec.ATOL + ec.P_RTOL * np.abs(a[1][:, :13, :13]), 10.0 * env_P)
    ex = np.abs(xg[:, :13] - a[0][:, :13])
    eP = np.abs(Pg[:, :13, :13] - a[1][:, :13, :13])
    ew = float(np.abs(ec.wind_entries(xg, Pg) - ec.wind_entries(a[0], a[1])).max())
    print(f"reference envelope: x13 {env_x:.3e} ({ec.worst(b[0][:, :13], a[0][:, :13], ec.X_RTOL):.2f} fixed bars), "
          f"P block {env_P:.3e} ({ec.worst(b[1][:, :13, :13], a[1][:, :13, :13], ec.P_RTOL):.2f} fixed bars), "
          f"wind entries {env_w:.3e}")
    print(f"gpu error: x13 {ex.max():.3e} ({(ex / bar_x).max():.3f} of its bar), P block {eP.max():.3e} "
          f"({(eP / bar_P).max():.3f}), wind entries {ew:.3e} (bar {bar_w:.3e})")
    assert np.all(ex <= bar_x)
    assert np.all(eP <= bar_P)
    assert ew <= bar_w


# ---- 8. the closed loop ---------------------------------------------------------------
def _fleet(ctrl_rows, estimator_model, steps=10):
    B, N = 8, 20
    cfg = ok.default_config(N=N)
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, B)
    try:
        ctx.plant_set_params(ec.rows_for(B))
        ctx.set_params(ctrl_rows)
        x0 = pc.states(B, 9500, N)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        kw = {} if estimator_model is None else dict(estimator_model=estimator_model)
        loop = FleetLoop(GpuStepper(ctx), torch.from_numpy(x0).cuda(), N, cfg.dt, wind_ekf=True,
                         covariances=ok.wind_ekf_default_covariances(), plant=GpuPlant(ctx, cfg.dt / 2, 2, 4), **kw)
        flags = 0
        for _ in range(steps):
            loop.step()
            torch.cuda.synchronize()
            flags |= int(np.bitwise_or.reduce(loop.ekf_status.cpu().numpy()))
        return dict(xe=loop.xe.cpu().numpy(), P=loop.P.cpu().numpy(), u0=loop.u0.cpu().numpy(),
                    x0=loop.x0.cpu().numpy(), flags=flags, plant=loop.plant_status.cpu().numpy(),
                    mode=ctx.estimator_model)
    finally:
        ctx.use_own_stream()
        ctx.close()


def test_fleet_loop_with_creation_rows_is_the_default_loop():
    a = _fleet(creation_rows(8), None)
    b = _fleet(creation_rows(8), "controller")
    assert (a["mode"], b["mode"]) == (ok.EST_MODEL_CREATION, ok.EST_MODEL_CONTROLLER)
    for key in ("xe", "P", "u0", "x0", "plant"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["flags"] == b["flags"]


def test_fleet_loop_filters_with_the_controllers_rows():
    rows = ec.rows_for(8)
    own = _fleet(rows, "controller")
    nom = _fleet(rows, "creation")
    assert not own["flags"] & ok.EKF_NAN
    assert not own["plant"].any()
    assert np.all(np.isfinite(own["xe"])) and np.all(np.isfinite(own["P"]))
    d = np.abs(own["xe"] - nom["xe"]).max(1)
    print("largest difference of the estimate per kite, controller's rows vs creation model:", np.round(d, 4))
    assert np.all(d > 0.0)


def test_fleet_loop_controller_model_needs_an_estimator():
    g = make(2)
    try:
        with pytest.raises(ValueError):
            FleetLoop(GpuStepper(g), torch.zeros((2, 15), dtype=torch.float64, device="cuda"), 20, 0.05,
                      estimator_model="controller")
        assert g.estimator_model == ok.EST_MODEL_CREATION
    finally:
        g.close()
