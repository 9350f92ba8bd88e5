"""The batched plant simulator (openkite_amd/csrc/plant_kernels.hip, k_plant;
kite_nmpc_plant_* in the C ABI): per-kite model parameters, a per-kite wind with
a sinusoidal gust, containment of non-finite kites, the FleetLoop and driver
wiring.

References: the CPU oracle's RK4 (ffi.rk4, any parameter vector, constant wind
through ffi.set_wind) and, for the gust, a Python RK4 over ffi.rhs_aug that sets
the wind W(t) = W0 + A sin(2 pi f t + phase) before every stage.

Bars, relative to max(1, |reference|) as test_gpu_parity.rel: the nominal plant
against kite_nmpc_predict 1e-12 (the same arithmetic; the constants arrive by
another path); against the oracle 1e-11 -- the project's bar for 4 RK4 steps is
1e-12 (test_gpu_parity.py), these runs take 12.  Every "continues", "device ==
host", "other kites" and closed-loop comparison is bitwise.
"""
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import FleetLoop, GpuPlant, GpuStepper
from oracle import ffi

from test_fleet import DT, N as N_ORACLE, OracleStepper, initial_states

B = 130                 # two full 64-lane blocks and a ragged third
H, STEPS, SUB = 0.02, 3, 4
HS = H / SUB
ORACLE_TOL = 1e-11
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "openkite_amd", "bin", "nmpf_driver")
PARAMS = os.path.join(REPO, "data", "umx_radian.yaml")


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def pad15(x13):
    x = np.zeros(x13.shape[:-1] + (15,))
    x[..., :13] = x13
    return x


def wind_at(w8, t):
    return w8[0:3] + w8[3:6] * math.sin(2.0 * math.pi * w8[6] * t + w8[7])


def oracle_const(kpb, x13, u4, n, w3=None):
    """ffi.rk4 over n substeps of HS, per kite with its own parameter row and wind."""
    out = np.zeros_like(x13)
    try:
        for b in range(x13.shape[0]):
            ffi.set_wind(None if w3 is None else w3[b])
            out[b] = ffi.rk4(kpb[b], pad15(x13[b]), u4[b], HS, n)[:13]
    finally:
        ffi.set_wind(None)
    return out


def oracle_gust(kpb, x13, u4, w8, t0, n):
    """RK4 in Python over ffi.rhs_aug, the wind set to W(t_stage) before each stage."""
    out = np.zeros_like(x13)
    try:
        for b in range(x13.shape[0]):
            x = pad15(x13[b])
            for k in range(n):
                t = t0 + k * HS
                acc, xs = x.copy(), x.copy()
                for st in range(4):
                    ts = t if st == 0 else (t + HS if st == 3 else t + 0.5 * HS)
                    ffi.set_wind(wind_at(w8[b], ts))
                    f = ffi.rhs_aug(kpb[b], xs, u4[b])
                    acc = acc + (HS / 6.0 if st in (0, 3) else HS / 3.0) * f
                    xs = x + (0.5 * HS if st < 2 else HS) * f
                x = acc
            out[b] = x[:13]
    finally:
        ffi.set_wind(None)
    return out


# ---- shared inputs and references (computed once, never modified) ------------
@pytest.fixture(scope="module")
def data(kp):
    rng = np.random.default_rng(4711)
    x13 = ffi.synthetic_states(B, offset=3000)
    u4 = np.zeros((B, 4))
    u4[:, 0] = rng.uniform(0.1, 0.15, B)
    u4[:, 1:3] = rng.uniform(-0.12, 0.12, (B, 2))
    u4[:, 3] = 0.7                                  # the plant ignores the virtual control
    P = ok.perturb_params(kp, B, 0.1, seed=7)
    w8 = np.zeros((B, 8))
    w8[:, 0:3] = rng.uniform(-0.5, 0.5, (B, 3)) / math.sqrt(3.0)      # |W0| <= 0.5 m/s
    w8[:, 3:6] = rng.uniform(-0.5, 0.5, (B, 3)) / math.sqrt(3.0)      # |A| <= 0.5 m/s
    w8[:, 6] = rng.uniform(0.5, 2.0, B)
    w8[:, 7] = rng.uniform(-math.pi, math.pi, B)
    for a in (x13, u4, P, w8):
        a.setflags(write=False)
    return dict(x13=x13, u4=u4, P=P, w8=w8, nominal=np.repeat(kp[None], B, axis=0))


@pytest.fixture(scope="module")
def ctx130():
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(), B)
    yield g
    g.close()


@pytest.fixture
def g(ctx130):
    ctx130.plant_set_params(None)
    ctx130.plant_set_wind(None)
    ctx130.use_own_stream()
    return ctx130


# ---- CPU: perturb_params -----------------------------------------------------
def test_perturb_params_is_seeded_and_selective(kp):
    a = ok.perturb_params(kp, 9, 0.1, seed=3)
    assert a.shape == (9, 52)
    np.testing.assert_array_equal(a, ok.perturb_params(ok.load_properties(), 9, 0.1, seed=3))
    assert not np.array_equal(a, ok.perturb_params(kp, 9, 0.1, seed=4))
    sel = [nmpc._PARAM_FIELDS.index(f) for f in ok.PERTURB_FIELDS]
    rest = [i for i in range(52) if i not in sel]
    # mass, the four inertias and the aerodynamic coefficients; geometry and tether untouched
    assert [nmpc._PARAM_FIELDS[i] for i in rest] == ["b", "c", "AR", "S", "lam", "St", "lt", "Sf", "lf", "Xac",
                                                     "Lt", "Ks", "Kd", "rx", "ry", "rz"]
    np.testing.assert_array_equal(a[:, rest], np.repeat(kp[None, rest], 9, axis=0))
    nz = [i for i in sel if kp[i] != 0.0]
    ratio = a[:, nz] / kp[nz]
    assert np.all(np.abs(ratio - 1.0) <= 0.1 + 4 * np.finfo(float).eps)      # within rel, up to the division's rounding
    assert np.all(ratio != 1.0) and ratio.std() > 0.03          # every selected field moved, per kite
    np.testing.assert_array_equal(a[:, [i for i in sel if kp[i] == 0.0]], 0.0)
    m = ok.perturb_params(kp, 5, 0.2, seed=1, fields=["mass"])
    assert np.all(m[:, nmpc._PARAM_FIELDS.index("mass")] != kp[10])
    m[:, 10] = kp[10]
    np.testing.assert_array_equal(m, np.repeat(kp[None], 5, axis=0))
    with pytest.raises(ValueError):
        ok.perturb_params(kp, 2, 0.1, seed=1, fields=["no_such_field"])


# ---- CPU: FleetLoop with a plant, on the oracle ------------------------------
class OraclePlant:
    """fleet.GpuPlant's interface on the CPU oracle: per-kite parameters and a
    constant per-kite wind (test only)."""

    def __init__(self, kpb, w3, h, steps, substeps):
        self.kpb, self.w3, self.h, self.steps, self.substeps = kpb, w3, h, steps, substeps
        self.calls = []

    def advance(self, x13, u0, t0, status):
        self.calls.append(t0)
        try:
            for b in range(x13.shape[0]):
                ffi.set_wind(self.w3[b])
                x = ffi.rk4(self.kpb[b], pad15(x13[b].numpy()), u0[b].numpy().copy(), self.h / self.substeps,
                            self.steps * self.substeps)
                x13[b] = torch.from_numpy(x[:13].copy())
        finally:
            ffi.set_wind(None)
        status.zero_()


def test_fleet_loop_flies_the_plant_not_the_plan(kp):
    nk, steps = 3, 4
    kpb = ok.perturb_params(kp, nk, 0.1, seed=11)
    w3 = np.array([[0.3, -0.2, 0.1], [0.0, 0.4, -0.1], [-0.3, 0.1, 0.2]])
    x_init = initial_states(0, nk)
    plant = OraclePlant(kpb, w3, DT / 2, 2, 4)
    loop = FleetLoop(OracleStepper(nk), x_init, N_ORACLE, DT, plant=plant)
    seen = []
    for s in range(steps):
        before = loop.xp.clone()
        loop.step()
        # the plant's own output, recomputed from the state before the step and the applied control
        want = before.clone()
        OraclePlant(kpb, w3, DT / 2, 2, 4).advance(want, loop.u0, 0.0, torch.zeros(nk, dtype=torch.int32))
        assert torch.equal(loop.x0[:, :13], want) and torch.equal(loop.xp, want)
        assert torch.equal(loop.x0[:, 13:], loop.traj[:, 1, 13:])
        assert not torch.equal(loop.x0[:, :13], loop.traj[:, 1, :13])      # not the plan's prediction
        seen.append(loop.x0.clone())
    assert plant.calls == pytest.approx([s * DT for s in range(steps)]) and loop.t == pytest.approx(steps * DT)
    assert torch.isfinite(torch.stack(seen)).all()
    loop.restart()
    assert loop.t == 0.0 and torch.equal(loop.xp, x_init[:, :13]) and torch.equal(loop.x0, x_init)
    again = []
    for s in range(steps):
        loop.step()
        again.append(loop.x0.clone())
    assert torch.equal(torch.stack(again), torch.stack(seen))


def test_fleet_loop_refuses_a_plant_period_that_is_not_dt(kp):
    kpb = np.repeat(kp[None], 3, axis=0)
    with pytest.raises(ValueError):
        FleetLoop(OracleStepper(3), initial_states(0, 3), N_ORACLE, DT, plant=OraclePlant(kpb, np.zeros((3, 3)), 0.02, 3, 4))
    FleetLoop(OracleStepper(3), initial_states(0, 3), N_ORACLE, DT, plant=OraclePlant(kpb, np.zeros((3, 3)), 0.0125, 4, 4))


# ---- GPU ------------------------------------------------------------------------
@pytest.mark.gpu
def test_nominal_plant_is_predict(g, data):
    want = g.predict(pad15(data["x13"]), data["u4"], H, SUB)[:, :13]
    got, st = g.plant_step(data["x13"], data["u4"], 0.0, H, steps=1, substeps=SUB)
    e = rel(got, want)
    print(f"nominal plant vs predict: rel {e:.2e}, bitwise {np.array_equal(got, want)}")
    assert e < 1e-12
    assert not st.any()
    assert not np.array_equal(got, data["x13"])


@pytest.fixture(scope="module")
def ref_perkite(data):
    return oracle_const(data["P"], data["x13"], data["u4"], STEPS * SUB)


@pytest.mark.gpu
def test_per_kite_parameters_match_the_oracle(g, data, ref_perkite):
    nominal, _ = g.plant_step(data["x13"], data["u4"], 0.0, H, STEPS, SUB)
    g.plant_set_params(data["P"])
    got, st = g.plant_step(data["x13"], data["u4"], 0.0, H, STEPS, SUB)
    e = rel(got, ref_perkite)
    print(f"per-kite parameters vs oracle: rel {e:.2e}")
    assert e < ORACLE_TOL and not st.any()
    # the parameters reach every kite
    assert np.abs(got - nominal).max(axis=1).min() > 1e-6
    # one plant model for all
    g.plant_set_params(data["P"][5])
    one, st = g.plant_step(data["x13"], data["u4"], 0.0, H, STEPS, SUB)
    want = oracle_const(np.repeat(data["P"][5:6], B, axis=0), data["x13"], data["u4"], STEPS * SUB)
    e1 = rel(one, want)
    print(f"count == 1 vs oracle: rel {e1:.2e}")
    assert e1 < ORACLE_TOL and not st.any()
    np.testing.assert_array_equal(one[5], got[5])
    # and back to the controller's own model
    g.plant_set_params(None)
    np.testing.assert_array_equal(g.plant_step(data["x13"], data["u4"], 0.0, H, STEPS, SUB)[0], nominal)


@pytest.mark.gpu
@pytest.mark.parametrize("perkite", [False, True])
def test_constant_wind_matches_the_oracle(g, data, perkite):
    kpb = data["P"] if perkite else data["nominal"]
    calm, _ = g.plant_step(data["x13"], data["u4"], 0.0, H, STEPS, SUB)
    if perkite:
        g.plant_set_params(data["P"])
    g.plant_set_wind(data["w8"][:, :3])
    got, st = g.plant_step(data["x13"], data["u4"], 0.0, H, STEPS, SUB)
    want = oracle_const(kpb, data["x13"], data["u4"], STEPS * SUB, data["w8"][:, :3])
    e = rel(got, want)
    print(f"constant wind (per-kite parameters: {perkite}) vs oracle: rel {e:.2e}")
    assert e < ORACLE_TOL and not st.any()
    assert np.abs(got - calm).max() > 1e-3                  # the wind is felt
    # a constant wind does not depend on the time
    np.testing.assert_array_equal(g.plant_step(data["x13"], data["u4"], 5.0, H, STEPS, SUB)[0], got)
    # an all-zero wind is no wind
    g.plant_set_wind(np.zeros((B, 3)))
    g.plant_set_params(None)
    np.testing.assert_array_equal(g.plant_step(data["x13"], data["u4"], 0.0, H, STEPS, SUB)[0], calm)


@pytest.mark.gpu
@pytest.mark.parametrize("perkite", [False, True])
def test_gust_matches_the_oracle_and_calls_continue(g, data, perkite):
    kpb = data["P"] if perkite else data["nominal"]
    w8 = data["w8"]
    if perkite:
        g.plant_set_params(data["P"])
    g.plant_set_wind(w8[:, :3])
    steady, _ = g.plant_step(data["x13"], data["u4"], 1.0, H, STEPS, SUB)
    g.plant_set_wind(w8[:, 0:3], w8[:, 3:6], w8[:, 6], w8[:, 7])
    got, st = g.plant_step(data["x13"], data["u4"], 1.0, H, STEPS, SUB)
    want = oracle_gust(kpb, data["x13"], data["u4"], w8, 1.0, STEPS * SUB)
    e = rel(got, want)
    print(f"gust (per-kite parameters: {perkite}) vs oracle: rel {e:.2e}; "
          f"gust moves the result by {np.abs(got - steady).max():.2e}")
    assert e < ORACLE_TOL and not st.any()
    assert np.abs(got - steady).max() > 1e-3                # the gust is felt, so it cannot be ignored
    # a second call at t0 = 1.06 continues the first: 3 + 3 steps == 6 steps, bitwise
    two, st2 = g.plant_step(got, data["u4"], 1.06, H, STEPS, SUB)
    six, st6 = g.plant_step(data["x13"], data["u4"], 1.0, H, 2 * STEPS, SUB)
    np.testing.assert_array_equal(two, six)
    assert not st2.any() and not st6.any()
    assert not np.array_equal(g.plant_step(got, data["u4"], 1.0, H, STEPS, SUB)[0], two)   # the time matters


def full_plant(g, data):
    g.plant_set_params(data["P"])
    g.plant_set_wind(data["w8"][:, 0:3], data["w8"][:, 3:6], data["w8"][:, 6], data["w8"][:, 7])


@pytest.mark.gpu
def test_device_and_host_entry_points_agree(g, data):
    full_plant(g, data)
    want, want_st = g.plant_step(data["x13"], data["u4"], 1.0, H, STEPS, SUB)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        x = torch.from_numpy(data["x13"].copy()).cuda()
        u = torch.from_numpy(data["u4"].copy()).cuda()
        st = torch.full((B,), 77, dtype=torch.int32, device="cuda")         # written, not OR-ed
        g.plant_step_device(x.data_ptr(), u.data_ptr(), 1.0, H, STEPS, SUB, st.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(x.cpu().numpy(), want)
        np.testing.assert_array_equal(st.cpu().numpy(), want_st)
        g.plant_step_device(x.data_ptr(), u.data_ptr(), 1.0, H, STEPS, SUB)       # the status is optional
        torch.cuda.synchronize()
        assert torch.isfinite(x).all()
    finally:
        g.use_own_stream()


@pytest.mark.gpu
def test_a_non_finite_kite_is_contained(g, data):
    full_plant(g, data)
    clean, clean_st = g.plant_step(data["x13"], data["u4"], 1.0, H, STEPS, SUB)
    assert not clean_st.any()
    x = data["x13"].copy()
    bad = {10: (0, np.nan), 70: (11, np.inf), 129: (6, -np.inf)}            # one per block, non-finite on entry
    for b, (col, v) in bad.items():
        x[b, col] = v
    x[3, 0] = 1e160                       # finite on entry, overflows in the first substep
    frozen = list(bad) + [3]
    got, st = g.plant_step(x, data["u4"], 1.0, H, STEPS, SUB)
    for b in frozen:
        assert np.array_equal(got[b], x[b], equal_nan=True), b
        assert st[b] == ok.PLANT_NAN, b
    others = [b for b in range(B) if b not in frozen]
    np.testing.assert_array_equal(got[others], clean[others])
    assert not st[others].any()
    # the status is written on every call: the same context, a clean batch again
    again, st = g.plant_step(data["x13"], data["u4"], 1.0, H, STEPS, SUB)
    np.testing.assert_array_equal(again, clean)
    assert not st.any()


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_change_nothing(g, data):
    def refused(call, *a, **k):
        with pytest.raises(ok.KiteNmpcError) as e:
            call(*a, **k)
        assert e.value.code == nmpc.KITE_EINVAL

    full_plant(g, data)
    want, _ = g.plant_step(data["x13"], data["u4"], 1.0, H, STEPS, SUB)
    refused(g.plant_set_params, data["P"][:B - 1])                       # count not in {1, B}
    refused(g.plant_set_params, data["P"][:2])
    for col, v in ((nmpc._PARAM_FIELDS.index("CLa_total"), np.nan), (nmpc._PARAM_FIELDS.index("Ks"), np.inf),
                   (nmpc._PARAM_FIELDS.index("mass"), 0.0), (nmpc._PARAM_FIELDS.index("mass"), -0.044)):
        P = data["P"].copy()
        P[B - 1, col] = v
        refused(g.plant_set_params, P)
        refused(g.plant_set_params, P[B - 1])
    P = data["P"].copy()
    for name, v in (("Ixx", 2.0), ("Izz", 8.0), ("Ixz", 4.0)):          # Ixx Izz - Ixz^2 == 0: singular inertia
        P[64, nmpc._PARAM_FIELDS.index(name)] = v
    refused(g.plant_set_params, P)
    for kw in (dict(h=0.0), dict(h=-0.02), dict(h=np.nan), dict(h=np.inf), dict(steps=0), dict(substeps=0),
               dict(t0=np.nan), dict(t0=np.inf), dict(steps=1 << 20, substeps=1 << 5)):
        a = dict(t0=1.0, h=H, steps=STEPS, substeps=SUB)
        a.update(kw)
        refused(g.plant_step, data["x13"], data["u4"], **a)
    w = data["w8"].copy()
    w[B - 1, 7] = np.nan
    refused(g.plant_set_wind, w[:, 0:3], w[:, 3:6], w[:, 6], w[:, 7])
    w = data["w8"].copy()
    w[0, 1] = np.inf
    refused(g.plant_set_wind, w[:, 0:3])
    # the plant set before the refused calls is still in force
    got, st = g.plant_step(data["x13"], data["u4"], 1.0, H, STEPS, SUB)
    np.testing.assert_array_equal(got, want)
    assert not st.any()


def _fleet_plant(nk, seed):
    rng = np.random.default_rng(seed)
    kp = ffi.load_params()
    P = ok.perturb_params(kp, nk, 0.1, seed=seed)
    d = rng.normal(size=(nk, 3))
    W0 = 0.5 * d / np.linalg.norm(d, axis=1, keepdims=True)             # 0.5 m/s, any direction
    A = rng.uniform(-0.2, 0.2, (nk, 3))
    return P, W0, A, rng.uniform(0.5, 2.0, nk), rng.uniform(-math.pi, math.pi, nk)


@pytest.mark.gpu
def test_closed_loop_on_the_device_equals_the_host_loop():
    from bench import synthetic_x0
    nk, Nh, steps = 16, 20, 6
    cfg = ok.default_config(N=Nh)
    h, psteps, sub = cfg.dt / 2, 2, 5
    plant = _fleet_plant(nk, 23)
    dev = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    host = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    try:
        for c in (dev, host):
            c.plant_set_params(plant[0])
            c.plant_set_wind(*plant[1:])
        x_init = synthetic_x0(nk, 0, dev)
        dev.set_stream(torch.cuda.current_stream().cuda_stream)
        loop = FleetLoop(GpuStepper(dev), torch.from_numpy(x_init).cuda(), Nh, cfg.dt,
                         plant=GpuPlant(dev, h, psteps, sub))
        x0, xp, t = x_init.copy(), x_init[:, :13].copy(), 0.0
        for s in range(steps):
            loop.step()
            r = host.step(x0)
            xp, pst = host.plant_step(xp, r["u0"], t, h, psteps, sub)
            t += cfg.dt
            x0 = np.concatenate([xp, r["traj"][:, 1, 13:]], axis=1)
            np.testing.assert_array_equal(loop.u0.cpu().numpy(), r["u0"], err_msg=f"step {s}")
            np.testing.assert_array_equal(loop.xp.cpu().numpy(), xp, err_msg=f"step {s}")
            np.testing.assert_array_equal(loop.x0.cpu().numpy(), x0, err_msg=f"step {s}")
            np.testing.assert_array_equal(loop.status.cpu().numpy(), r["status"], err_msg=f"step {s}")
            assert not pst.any() and not loop.plant_status.cpu().numpy().any(), s
            assert not (r["status"] & nmpc.ST_NAN).any(), s
            # the plant is not the plan
            assert np.abs(xp - r["traj"][:, 1, :13]).max() > 1e-4
        assert loop.t == t and np.all(np.isfinite(x0))
    finally:
        dev.close()
        host.close()


@pytest.mark.gpu
def test_driver_flies_the_plant_files(tmp_path):
    nk, S, K = 8, 5, 3
    P, W0, A, f, ph = _fleet_plant(nk, 31)
    w8 = np.concatenate([W0, A, f[:, None], ph[:, None]], axis=1)
    x13 = ffi.synthetic_states(nk, offset=970)
    for name, a in (("x0", x13), ("pp", P), ("pw", w8)):
        np.savetxt(tmp_path / f"{name}.csv", a, delimiter=",", fmt="%.17g")
    out = subprocess.run([DRIVER, "--params", PARAMS, "--batch", str(nk), "--steps", str(S), "--x0", str(tmp_path / "x0.csv"),
                          "--ctrl-every", str(K), "--sim-dt", str(H), "--delay", "0.1", "--trace", str(nk),
                          "--plant-params", str(tmp_path / "pp.csv"), "--plant-wind", str(tmp_path / "pw.csv")],
                         check=True, capture_output=True, text=True).stdout
    recs = [json.loads(l) for l in out.strip().splitlines()]
    diag = {(r["step"], r["kite"]): r for r in recs if r["type"] == "mpc_diagnostic"}
    summary = [r for r in recs if r["type"] == "step"]
    assert len(summary) == S and all(r["plant_nan"] == 0 and r["nan"] == 0 for r in summary)
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(delay=0.1, delay_steps=16), nk)
    try:
        g.plant_set_params(P)
        g.plant_set_wind(W0, A, f, ph)
        plant, t, traj = x13.copy(), 0.0, None
        theta = g.closest_point(plant[:, 6:9], np.zeros(nk))
        for s in range(S):
            x0 = np.zeros((nk, 15))
            x0[:, :13] = plant
            x0[:, 13] = theta if s == 0 else traj[:, 1, 13]
            x0[:, 14] = 0.0 if s == 0 else traj[:, 1, 14]
            r = g.step(x0)
            traj = r["traj"]
            for b in range(nk):
                np.testing.assert_array_equal(np.array(diag[(s, b)]["x"]), plant[b], err_msg=f"step {s} kite {b}")
                np.testing.assert_array_equal(np.array(diag[(s, b)]["u"]), r["u0"][b])
            u4 = r["u0"].copy()
            u4[:, 3] = 0.0
            plant, st = g.plant_step(plant, u4, t, H, K, 4)
            assert not st.any()
            for _ in range(K):
                t += H
            assert summary[s]["t"] == pytest.approx(t - K * H, abs=1e-4)
    finally:
        g.close()
