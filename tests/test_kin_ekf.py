"""The kinematic (pose-only) EKF on the GPU: k_ekf_kin, k_ekf_kin_init and
k_jacobian_kin against the numpy reference (tests/kin_ekf_ref.py, itself
checked on the CPU by tests/test_kin_ekf_ref.py), the bitwise properties of the
fused call, containment of bad kites, the Python mirror and the fleet loop.

Bars: the filter's are tests/test_ekf.py's (x rtol 1e-12, P rtol 1e-11, both
atol 1e-13).  The Jacobian and the initialisation are held to rtol 1e-13 entry
by entry (measured: 2.4e-14 and 4.0e-15 at worst)."""
import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import FleetLoop, FlightRecorder, GpuPlant, GpuStepper
from oracle import ffi
from tests import kin_ekf_ref as ref
from tests import perkite_cases as pc
from tests import test_kin_ekf_ref as cpu

pytestmark = pytest.mark.gpu

K = 4                                   # kites per block of k_ekf_kin
SHAPES = [1, K - 1, K, K + 1, 2 * K + 1]
DT = 0.02


@pytest.fixture(scope="module")
def ctx():
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(), 1)
    yield g
    g.close()


def unframe(zw, fr):
    """The motion-capture pose whose frame change is the world pose zw (unit rotation)."""
    off, rot, sh = (np.asarray(fr[k], dtype=np.float64) for k in ("offset", "rotation", "shift"))
    q = ref.qmul(ref.qmul(ref.conj(rot), zw[3:]), rot)
    r = ref.rotate(ref.conj(rot), zw[:3] - sh) - ref.rotate(q, off)
    return np.r_[r, q]


def inputs(B, seed=3, framed=False):
    """x, P, z, W, V as tests/test_ekf.py's _inputs; framed: z as the motion capture sees it."""
    rng = np.random.default_rng(seed)
    x = ffi.synthetic_states(B, offset=600)
    W, V, P0 = ok.ekf_default_covariances()
    G = rng.normal(size=(B, 13, 13)) * 0.01
    P = np.repeat(P0[None], B, axis=0) + G @ G.transpose(0, 2, 1)     # a generic SPD covariance
    z = x[:, 6:13] + rng.normal(size=(B, 7)) * 0.01
    if framed:
        z = np.array([unframe(zb, ref.DEFAULT_FRAME) for zb in z])
    return x, P, z, W, V


def reference(x, P, dt, substeps, z, W, V, fr, **kw):
    out = [ref.step(x[b], P[b], dt, substeps, None if z is None else z[b], W, V, fr, **kw) for b in range(len(x))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


# ---- the Jacobian pass and the filter against the reference ------------------------
@pytest.mark.parametrize("B", SHAPES)
def test_jacobian_kin_vs_reference(ctx, B):
    x = cpu.seeded_states(B)
    J = ctx.jacobian_kin(x)
    worst = 0.0
    for b in range(B):
        Jr = ref.jac(x[b])
        nz = Jr != 0.0
        worst = max(worst, (np.abs(J[b] - Jr)[nz] / np.abs(Jr[nz])).max())
    print(f"B={B}: jacobian_kin, worst entry-wise relative error {worst:.2e}")
    for b in range(B):
        Jr = ref.jac(x[b])
        np.testing.assert_allclose(J[b], Jr, rtol=1e-13, atol=0.0)
        np.testing.assert_array_equal(J[b][Jr == 0.0], 0.0)          # the structural zeros are zeros


@pytest.mark.parametrize("B", SHAPES)
def test_filter_vs_reference(ctx, B):
    worst = [0.0, 0.0]
    for substeps in (1, 5):
        for update in (False, True):
            for framed in (False, True):
                x, P, z, W, V = inputs(B, framed=framed)
                fr = ref.DEFAULT_FRAME if framed else None
                xg, Pg, st = ctx.kin_ekf_step(x, P, DT, substeps, z if update else None, W, V,
                                              ok.pose_frame_default() if framed else None)
                xr, Pr, sr = reference(x, P, DT, substeps, z if update else None, W, V, fr)
                case = (substeps, update, framed)
                np.testing.assert_array_equal(st, sr, err_msg=str(case))
                assert not st.any()
                worst[0] = max(worst[0], (np.abs(xg - xr) / (1e-13 + 1e-12 * np.abs(xr))).max())
                worst[1] = max(worst[1], (np.abs(Pg - Pr) / (1e-13 + 1e-11 * np.abs(Pr))).max())
                np.testing.assert_allclose(xg, xr, rtol=1e-12, atol=1e-13, err_msg=str(case))
                np.testing.assert_allclose(Pg, Pr, rtol=1e-11, atol=1e-13, err_msg=str(case))
                if update:
                    np.testing.assert_array_equal(Pg, Pg.transpose(0, 2, 1))       # exactly symmetric
    print(f"B={B}: worst error in units of the bar: x {worst[0]:.3f}, P {worst[1]:.3f}")


def test_null_frame_and_identity_frame(ctx):
    """NULL is taken as given; the identity frame agrees with it to rounding."""
    x, P, z, W, V = inputs(5)
    a = ctx.kin_ekf_step(x, P, DT, 5, z, W, V, None)
    b = ctx.kin_ekf_step(x, P, DT, 5, z, W, V, ref.IDENTITY_FRAME)
    np.testing.assert_allclose(b[0], a[0], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(b[1], a[1], rtol=1e-11, atol=1e-13)
    # taken as given: a z already equal to the propagated pose leaves the estimate there, bit for bit
    xp, _, _ = ctx.kin_ekf_step(x, P, DT, 5, None, W, V, None)
    xu, _, _ = ctx.kin_ekf_step(x, P, DT, 5, xp[:, 6:13].copy(), W, V, None)
    np.testing.assert_array_equal(xu, xp)


# ---- bitwise properties -------------------------------------------------------------
@pytest.mark.parametrize("framed", [False, True])
def test_fused_equals_unfused_bitwise(ctx, framed):
    x, P, z, W, V = inputs(5, framed=framed)
    fr = ok.pose_frame_default() if framed else None
    xf, Pf, sf = ctx.kin_ekf_step(x, P, DT, 5, z, W, V, fr)
    xu, Pu = x, P
    for k in range(5):
        xu, Pu, su = ctx.kin_ekf_step(xu, Pu, DT / 5, 1, z if k == 4 else None, W, V, fr)
    np.testing.assert_array_equal(xf, xu)
    np.testing.assert_array_equal(Pf, Pu)
    np.testing.assert_array_equal(sf, su)


@pytest.mark.parametrize("framed", [False, True])
def test_measured_quaternion_sign_is_immaterial_bitwise(ctx, framed):
    x, P, z, W, V = inputs(5, framed=framed)
    fr = ok.pose_frame_default() if framed else None
    zn = z.copy(); zn[:, 3:] = -zn[:, 3:]
    a = ctx.kin_ekf_step(x, P, DT, 5, z, W, V, fr)
    b = ctx.kin_ekf_step(x, P, DT, 5, zn, W, V, fr)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    # and the flipped stream is not read as an attitude half a turn away
    np.testing.assert_allclose(b[0][:, 9:13], x[:, 9:13], atol=0.1)


def test_device_call_leaves_the_callers_z(ctx):
    x, P, z, W, V = inputs(9, framed=True)
    fr = ok.pose_frame_default()
    xh, Ph, sh = ctx.kin_ekf_step(x, P, DT, 5, z, W, V, fr)
    dev = [torch.from_numpy(a.copy()).cuda() for a in (x, P, z, W, V)]
    st = torch.full((9,), -1, dtype=torch.int32, device="cuda")
    ctx.kin_ekf_step_device(9, DT, 5, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                            dev[4].data_ptr(), st.data_ptr(), frame=fr)
    ctx.synchronize()
    np.testing.assert_array_equal(dev[2].cpu().numpy(), z)            # the caller's z
    np.testing.assert_array_equal(dev[0].cpu().numpy(), xh)
    np.testing.assert_array_equal(dev[1].cpu().numpy(), Ph)
    np.testing.assert_array_equal(st.cpu().numpy(), sh)


# ---- containment ------------------------------------------------------------------------
def test_bad_kites_are_contained():
    B = 5
    x, P, z, W, V = inputs(B)
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(), 1)
    try:
        clean = g.kin_ekf_step(x, P, DT, 5, z, W, V)
        prop = g.kin_ekf_step(x, P, DT, 5, None, W, V)
        xb, Pb, zb = x.copy(), P.copy(), z.copy()
        xb[1, 4] = np.nan                    # a NaN estimate
        Pb[2, 7, 3] = np.nan                 # a NaN covariance
        zb[4, 5] = np.nan                    # a NaN measurement: a bad update, not a NaN kite
        xg, Pg, st = g.kin_ekf_step(xb, Pb, DT, 5, zb, W, V)
        np.testing.assert_array_equal(st, [0, ok.EKF_NAN, ok.EKF_NAN, 0, ok.EKF_S_NOT_PD])
        for b in (1, 2):                     # kept bitwise
            np.testing.assert_array_equal(xg[b], xb[b])
            np.testing.assert_array_equal(Pg[b], Pb[b])
        np.testing.assert_array_equal(xg[4], prop[0][4])              # the propagated estimate
        np.testing.assert_array_equal(Pg[4], prop[1][4])
        for b in (0, 3):                     # the block neighbours: as without the bad kites
            np.testing.assert_array_equal(xg[b], clean[0][b])
            np.testing.assert_array_equal(Pg[b], clean[1][b])
        # status words are written, not OR-ed: the same arrays, healthy again
        assert not g.kin_ekf_step(x, P, DT, 5, z, W, V)[2].any()
    finally:
        g.close()


def test_s_not_positive_definite_keeps_the_propagated_estimate():
    """V = -I makes every kite's S indefinite (V is shared): run as its own case."""
    B = 5
    x, P, z, W, V = inputs(B)
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(), 1)
    try:
        prop = g.kin_ekf_step(x, P, DT, 5, None, W, V)
        xg, Pg, st = g.kin_ekf_step(x, P, DT, 5, z, W, -np.eye(7))
        np.testing.assert_array_equal(st, [ok.EKF_S_NOT_PD] * B)
        np.testing.assert_array_equal(xg, prop[0])
        np.testing.assert_array_equal(Pg, prop[1])
        _, _, sr = reference(x, P, DT, 5, z, W, -np.eye(7), None)
        np.testing.assert_array_equal(sr, st)
    finally:
        g.close()


# ---- the two-pose initialisation -------------------------------------------------------
def _poses(B, seed=4):
    rng = np.random.default_rng(seed)
    x = ffi.synthetic_states(B, offset=650)
    prev = x[:, 6:13].copy()
    new = np.array([ref.rk4(xb, DT) for xb in x])[:, 6:13] + rng.normal(size=(B, 7)) * 1e-3
    new[::2, 3:] *= -1.0                    # a stream that flips its quaternion sign
    return prev, new


@pytest.mark.parametrize("framed", [False, True])
@pytest.mark.parametrize("B", SHAPES)
def test_init_vs_reference(ctx, B, framed):
    prev, new = _poses(B)
    xg, st = ctx.kin_ekf_init(prev, new, DT, ok.pose_frame_default() if framed else None)
    assert not st.any()
    worst = 0.0
    for b in range(B):
        xr, sr = ref.init(prev[b], new[b], DT, ref.DEFAULT_FRAME if framed else None)
        assert sr == 0
        worst = max(worst, (np.abs(xg[b] - xr) / np.abs(xr)).max())
        np.testing.assert_allclose(xg[b], xr, rtol=1e-13, atol=0.0, err_msg=str(b))
        if not framed:
            np.testing.assert_array_equal(xg[b, 6:], new[b])         # the pose as measured
    print(f"B={B} framed={framed}: kin_ekf_init, worst entry-wise relative error {worst:.2e}")


def test_init_flags_what_it_cannot_initialise(ctx):
    B = 5
    prev, new = _poses(B)
    keep = np.arange(B * 13, dtype=np.float64).reshape(B, 13)
    good, _ = ctx.kin_ekf_init(prev, new, DT, None, keep)
    x0, st0 = ctx.kin_ekf_init(prev, new, 0.0, None, keep)           # dt = 0: every kite
    np.testing.assert_array_equal(st0, [ok.EKF_INIT_BAD] * B)
    np.testing.assert_array_equal(x0, keep)
    bad = new.copy(); bad[1, 2] = np.nan
    x1, st1 = ctx.kin_ekf_init(prev, bad, DT, None, keep)            # one NaN pose
    np.testing.assert_array_equal(st1, [0, ok.EKF_INIT_BAD, 0, 0, 0])
    np.testing.assert_array_equal(x1[1], keep[1])
    np.testing.assert_array_equal(np.delete(x1, 1, 0), np.delete(good, 1, 0))


@pytest.mark.parametrize("framed", [False, True])
def test_init_host_equals_device(ctx, framed):
    """kin_ekf_init and kin_ekf_init_device at count 5, one pose non-finite: the same bits."""
    B = 5
    prev, new = _poses(B)
    new[3, 1] = np.nan
    fr = ok.pose_frame_default() if framed else None
    keep = np.arange(B * 13, dtype=np.float64).reshape(B, 13)
    xh, sh = ctx.kin_ekf_init(prev, new, DT, fr, keep)
    dp, dn, dx = (torch.from_numpy(a.copy()).cuda() for a in (prev, new, keep))
    st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ctx.kin_ekf_init_device(B, DT, dp.data_ptr(), dn.data_ptr(), dx.data_ptr(), st.data_ptr(), frame=fr)
    ctx.synchronize()
    np.testing.assert_array_equal(sh, [0, 0, 0, ok.EKF_INIT_BAD, 0])
    np.testing.assert_array_equal(dx.cpu().numpy(), xh)
    np.testing.assert_array_equal(st.cpu().numpy(), sh)


def test_bad_arguments(ctx):
    x, P, z, W, V = inputs(2)

    def refused(fn):
        with pytest.raises(ok.KiteNmpcError) as e:
            fn()
        assert e.value.code == nmpc.KITE_EINVAL

    refused(lambda: ctx.kin_ekf_step(np.zeros((0, 13)), np.zeros((0, 13, 13)), DT, 1, None, W, V))
    for dt in (0.0, -DT, np.nan, np.inf):
        refused(lambda: ctx.kin_ekf_step(x, P, dt, 1, z, W, V))
    for substeps in (0, -1, 2 ** 24 + 1):
        refused(lambda: ctx.kin_ekf_step(x, P, DT, substeps, z, W, V))
    for rot in ((0.0, 0.0, 0.0, 0.0), (np.nan, 1.0, 0.0, 0.0), (np.inf, 0.0, 0.0, 0.0)):
        fr = dict(ref.DEFAULT_FRAME, rotation=rot)
        refused(lambda: ctx.kin_ekf_step(x, P, DT, 1, z, W, V, fr))
        refused(lambda: ctx.kin_ekf_init(z, z, DT, fr))
    refused(lambda: ctx.kin_ekf_init(np.zeros((0, 7)), np.zeros((0, 7)), DT))
    refused(lambda: ctx.jacobian_kin(np.zeros((0, 13))))
    # nothing above touched the filter: the arrays still give a clean step
    assert not ctx.kin_ekf_step(x, P, DT, 1, z, W, V)[2].any()


# ---- the mirror ------------------------------------------------------------------------------
def test_kite_ekf_mirror_kinematic_open_loop():
    """tests/test_kin_ekf_ref.py's open-loop scenario through KiteEKF(B,
    model="kinematic"): the same bar, finite P."""
    s = cpu.OPEN_LOOP
    truth, zs, est0 = cpu.open_loop_data()
    ekf = ok.KiteEKF(s["B"], model="kinematic", substeps=s["substeps"])
    try:
        ekf.setEstimation(est0)
        ekf.setControl(np.tile([0.12, 0.0, 0.0], (s["B"], 1)))        # accepted and ignored
        err0 = np.abs(ekf.getEstimation() - truth[0])[:, :3].mean()
        t = 0.0
        for k in range(s["periods"]):
            t += s["dt"]
            ekf.estimate(zs[k], t)
            ekf.setTime(t)
            assert not ekf.status.any()
        err1 = np.abs(ekf.getEstimation() - truth[-1])[:, :3].mean()
        print(f"open loop on the GPU: mean |v_b error| {err0:.4f} -> {err1:.4f}, ratio {err1 / err0:.3f}")
        assert np.all(np.isfinite(ekf.getEstimationCovariance()))
        assert err1 < 0.5 * err0, (err0, err1)
        # initialize: the node's two poses
        ekf.initialize(truth[0][:, 6:13], truth[1][:, 6:13], s["dt"])
        assert not ekf.status.any()
        np.testing.assert_array_equal(ekf.getEstimation()[:, 6:], truth[1][:, 6:13])
        assert np.abs(ekf.getEstimation()[:, :6] - truth[1][:, :6]).max() < 0.5
    finally:
        ekf.close()
    with pytest.raises(ValueError):
        ok.KiteEKF(1, model="kinetic")


# ---- the fleet loop ----------------------------------------------------------------------------
def _fleet(steps=10, **kw):
    B, N = 16, 20
    cfg = ok.default_config(N=N)
    g = ok.BatchNMPC(ok.load_properties(), cfg, B)
    try:
        g.plant_set_params(ok.perturb_params(g.params, B, 0.1, seed=21))
        x0 = pc.states(B, 9600, N)
        g.set_stream(torch.cuda.current_stream().cuda_stream)
        rec = FlightRecorder(B, steps, "cuda")
        if kw.get("kin_ekf"):
            kw["covariances"] = ok.ekf_default_covariances()
        loop = FleetLoop(GpuStepper(g), torch.from_numpy(x0).cuda(), N, cfg.dt, plant=GpuPlant(g, cfg.dt / 2, 2, 4),
                         recorder=rec, **kw)
        est, flags = [], 0
        for _ in range(steps):
            loop.step()
            torch.cuda.synchronize()
            if kw.get("kin_ekf"):
                flags |= int(np.bitwise_or.reduce(loop.ekf_status.cpu().numpy()))
                est.append(loop.xe.cpu().numpy().copy())      # the estimate this step's RTI started from
        return dict(x_launch=x0, X=rec.X.cpu().numpy(), U=rec.U.cpu().numpy(), x0=loop.x0.cpu().numpy(),
                    u0=loop.u0.cpu().numpy(), est=est, flags=flags, status=loop.status.cpu().numpy(),
                    plant=loop.plant_status.cpu().numpy(), P=loop.P.cpu().numpy() if kw.get("kin_ekf") else None)
    finally:
        g.use_own_stream()
        g.close()


def test_fleet_loop_with_the_kinematic_filter():
    r = _fleet(kin_ekf=True)
    print("RTI status words of the last step:", sorted(set(r["status"].tolist())))
    assert r["flags"] == 0 and not r["plant"].any() and not r["status"].any()
    for key in ("X", "U", "x0", "u0", "P"):
        assert np.all(np.isfinite(r[key])), key
    np.testing.assert_array_equal(r["X"][:, 0, :], r["x_launch"][:, :13])        # the first step filters nothing
    for k in range(10):                                                          # the log is the estimate
        np.testing.assert_array_equal(r["X"][:, k, :], r["est"][k])
    assert np.abs(r["X"][:, 1:10, :] - r["X"][:, :1, :]).max() > 0.0


def test_fleet_loop_without_the_keyword_is_what_it_was():
    a = _fleet()
    b = _fleet(kin_ekf=False)
    for key in ("X", "U", "x0", "u0", "status", "plant"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def test_fleet_loop_refusals(ctx):
    x0 = torch.zeros((2, 15), dtype=torch.float64, device="cuda")
    cov = ok.ekf_default_covariances()
    st = GpuStepper(ctx)
    with pytest.raises(ValueError):
        FleetLoop(st, x0, 20, 0.05, kin_ekf=True, ekf=True, covariances=cov)
    with pytest.raises(ValueError):
        FleetLoop(st, x0, 20, 0.05, kin_ekf=True, wind_ekf=True, covariances=ok.wind_ekf_default_covariances())
    with pytest.raises(ValueError):
        FleetLoop(st, x0, 20, 0.05, kin_ekf=True, covariances=cov, estimator_model="controller")
    assert ctx.estimator_model == ok.EST_MODEL_CREATION
    with pytest.raises(ValueError):          # ident_wind="estimate" still needs the wind EKF
        FleetLoop(st, x0, 20, 0.05, kin_ekf=True, covariances=cov, ident_wind="estimate",
                  recorder=FlightRecorder(2, 4, "cuda", wind=True))
    with pytest.raises(ValueError):
        FleetLoop(st, x0, 20, 0.05, kin_ekf=True)      # no covariances
    # restart resets the filter
    loop = FleetLoop(st, x0, 20, 0.05, kin_ekf=True, covariances=cov)
    loop.kin_ekf_fresh = False
    loop.xe.fill_(1.0); loop.P.fill_(2.0); loop.ekf_status.fill_(3)
    loop.restart()
    assert loop.kin_ekf_fresh and not loop.ekf_status.any().item()
    assert torch.equal(loop.xe, x0[:, :13]) and torch.equal(loop.P, loop.P_init)
