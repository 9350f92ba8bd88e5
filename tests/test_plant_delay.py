"""The plant behind a per-kite command line (k_plant_delay in
openkite_amd/csrc/plant_kernels.hip; kite_nmpc_plant_step_delayed[_device];
fleet.ActuationDelay / GpuPlant(delay=) / FleetLoop; nmpf_driver --plant-delay).

Every comparison is bitwise.  The expected line, u_applied and status bits come
from the pure-Python model tests/delay_ref.py.  The expected state is composed
on the GPU from the existing, undelayed kite_nmpc_plant_step(steps=1): the
controls the model says are in force, given plant step by plant step at the
host's step times t0 + float(j * substeps) * hs (test_plant.py pins that such
chained calls continue each other).  For the gust the composition goes substep
by substep (steps=1, substeps=1, h=hs, at t0 + float(k) * hs): the gust reads
the time, and (t0 + a hs) + m hs is not t0 + (a + m) hs in floating point (8 of
this file's 96 substep times differ in the last bit), whereas a call with one
substep starts exactly at the time the single launch computes.

Shapes: B = 70 (two 64-lane blocks, the second partial), 3 plant steps of 2
substeps per period, 8 consecutive periods.
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
from openkite_amd.fleet import ActuationDelay, EpisodeScore, FleetLoop, FlightRecorder, GpuPlant, GpuStepper
from oracle import ffi

import delay_ref as dr

pytestmark = pytest.mark.gpu

B = 70
H, STEPS, SUB, PERIODS = 0.02, 3, 2, 8
HS, DT = H / SUB, STEPS * H
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "openkite_amd", "bin", "nmpf_driver")
PARAMS = os.path.join(REPO, "data", "umx_radian.yaml")
# (b): on the tick, inside a step, across a step, one period, the node's two, across periods, beyond the depth
TAU_CYCLE = np.array([0.0, 0.5 * H, 1.3 * H, DT, 2 * DT, 2.4 * DT, 4.7 * DT])


@pytest.fixture(scope="module")
def data(kp):
    rng = np.random.default_rng(2718)
    x13 = ffi.synthetic_states(B, offset=4000)
    u = np.zeros((PERIODS, B, 4))
    u[:, :, 0] = rng.uniform(0.1, 0.15, (PERIODS, B))
    u[:, :, 1:3] = rng.uniform(-0.12, 0.12, (PERIODS, B, 2))
    u[:, :, 3] = rng.uniform(-1.0, 1.0, (PERIODS, B))          # carried by the line, ignored by the plant
    P = ok.perturb_params(kp, B, 0.1, seed=9)
    w8 = np.zeros((B, 8))
    w8[:, 0:3] = rng.uniform(-0.5, 0.5, (B, 3)) / math.sqrt(3.0)
    w8[:, 3:6] = rng.uniform(-0.5, 0.5, (B, 3)) / math.sqrt(3.0)
    w8[:, 6] = rng.uniform(0.5, 2.0, B)
    w8[:, 7] = rng.uniform(-math.pi, math.pi, B)
    tau_b = np.tile(TAU_CYCLE[np.arange(B) % len(TAU_CYCLE)], (PERIODS, 1))
    for a in (x13, u, P, w8, tau_b):
        a.setflags(write=False)
    return dict(x13=x13, u=u, P=P, w8=w8, tau_b=tau_b)


@pytest.fixture(scope="module")
def ctx70():
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(), B)
    yield g
    g.close()


@pytest.fixture
def g(ctx70):
    ctx70.plant_set_params(None)
    ctx70.plant_set_wind(None)
    ctx70.use_own_stream()
    return ctx70


def set_plant(g, P, w8, perkite, wind):
    """wind: 0 calm, 1 constant, 2 gust (k_plant's WIND)."""
    g.plant_set_params(P if perkite else None)
    if wind == 1:
        g.plant_set_wind(w8[:, 0:3])
    elif wind == 2:
        g.plant_set_wind(w8[:, 0:3], w8[:, 3:6], w8[:, 6], w8[:, 7])
    else:
        g.plant_set_wind(None)


def compose(g, x, u_steps, t0, by_substep):
    """The period flown with the undelayed plant_step(steps=1), the control of
    every plant step given; returns (x, OR of the status words)."""
    st = np.zeros(x.shape[0], dtype=np.int32)
    for j in range(STEPS):
        if by_substep:
            for m in range(SUB):
                x, s = g.plant_step(x, u_steps[j], t0 + float(j * SUB + m) * HS, HS, 1, 1)
                st |= s
        else:
            x, s = g.plant_step(x, u_steps[j], t0 + float(j * SUB) * HS, H, 1, SUB)
            st |= s
    return x, st


def fly(g, x13, u, tau, by_substep=False, send=lambda p: True):
    """PERIODS delayed calls against the model and the composed plant, every
    output compared bitwise each period; returns the per-period outputs."""
    nk = x13.shape[0]
    ref = dr.Fleet(nk)
    x, xr = x13.copy(), x13.copy()
    line = np.zeros((nk, ok.DELAY_NLINE))
    out, t = [], 0.0
    for p in range(PERIODS):
        cmd = u[p] if send(p) else None
        x, line, ua, st = g.plant_step_delayed(x, cmd, tau[p] if cmd is not None else None, line, t, H, STEPS, SUB)
        u_steps, rows, ua_ref, bits = ref.call(cmd, tau[p], t, H, STEPS, SUB)
        xr, nan_bits = compose(g, xr, u_steps, t, by_substep)
        np.testing.assert_array_equal(line, rows, err_msg=f"line, period {p}")
        np.testing.assert_array_equal(ua, ua_ref, err_msg=f"u_applied, period {p}")
        np.testing.assert_array_equal(st, bits | nan_bits, err_msg=f"status, period {p}")
        assert np.array_equal(x, xr, equal_nan=True), f"state, period {p}: {np.nanmax(np.abs(x - xr)):.3e}"
        out.append(dict(x=x.copy(), line=line.copy(), ua=ua.copy(), st=st.copy(), u_steps=u_steps))
        t += DT
    return out


# ---- (a) zero latency ----------------------------------------------------------
def test_zero_latency_is_the_undelayed_plant(g, data):
    out = fly(g, data["x13"], data["u"], np.zeros((PERIODS, B)))
    x, t = data["x13"].copy(), 0.0
    for p in range(PERIODS):
        x, st = g.plant_step(x, data["u"][p], t, H, STEPS, SUB)       # one undelayed launch per period
        np.testing.assert_array_equal(out[p]["x"], x, err_msg=f"period {p}")
        np.testing.assert_array_equal(out[p]["ua"], data["u"][p])
        assert not out[p]["st"].any() and not st.any() and not out[p]["line"][:, nmpc.DELAY_COUNT].any()
        t += DT


# ---- (b) per-kite latencies, (g) in all six variants ---------------------------
@pytest.mark.parametrize("wind", [0, 1, 2])
@pytest.mark.parametrize("perkite", [False, True])
def test_per_kite_latencies_in_every_variant(g, data, perkite, wind):
    set_plant(g, data["P"], data["w8"], perkite, wind)
    out = fly(g, data["x13"], data["u"], data["tau_b"], by_substep=wind == 2)
    dropped = np.zeros(B, dtype=bool)
    for o in out:
        dropped |= (o["st"] & ok.PLANT_CMD_DROPPED) != 0
        assert not (o["st"] & (ok.PLANT_NAN | ok.PLANT_BAD_TAU)).any()
    beyond = np.arange(B) % len(TAU_CYCLE) == 6                         # 4.7 periods: the depth overflows
    assert dropped[beyond].all() and not dropped[np.arange(B) % len(TAU_CYCLE) < 4].any()
    # the latencies are felt: from one period on, the last command has not arrived by the last tick
    assert np.abs(out[-1]["ua"] - data["u"][-1]).max(axis=1)[np.arange(B) % len(TAU_CYCLE) >= 3].min() > 0
    np.testing.assert_array_equal(out[-1]["ua"][np.arange(B) % len(TAU_CYCLE) < 3], data["u"][-1][np.arange(B) % len(TAU_CYCLE) < 3])
    # a command that arrives inside a period changes the control between its steps
    assert any((o["u_steps"][0] != o["u_steps"][-1]).any() for o in out)


# ---- (c) FIFO ------------------------------------------------------------------
def test_the_line_never_reorders(g, data):
    fall = np.array([3.2, 2.1, 1.0, 0.3, 0.0, 0.0, 0.0, 0.0]) * DT        # raw arrivals 3.2, 3.1, 3.0, 3.3 periods
    scale = 1.0 + 0.01 * (np.arange(B) % 5)
    tau = fall[:, None] * scale[None, :]
    assert np.any(np.diff(np.arange(PERIODS)[:, None] * DT + tau, axis=0) < 0)      # they would reorder
    out = fly(g, data["x13"], data["u"], tau)
    for o in out:
        n = o["line"][:, nmpc.DELAY_COUNT].astype(int)
        for b in range(B):
            assert np.all(np.diff(o["line"][b, nmpc.DELAY_T_ARR:nmpc.DELAY_T_ARR + n[b]]) >= 0)
    np.testing.assert_array_equal(out[-1]["ua"], data["u"][-1])                     # everything got through, in order


# ---- (d) coast -----------------------------------------------------------------
def test_periods_without_a_command_coast(g, data):
    tau = np.full((PERIODS, B), 1.3 * H)
    out = fly(g, data["x13"], data["u"], tau, send=lambda p: p % 2 == 0)
    np.testing.assert_array_equal(out[1]["ua"], data["u"][0])                       # period 1 flies period 0's command
    np.testing.assert_array_equal(out[-1]["ua"], data["u"][PERIODS - 2])


# ---- (e) bad tau ---------------------------------------------------------------
def test_a_bad_tau_drops_the_command_and_spares_the_neighbours(g, data):
    set_plant(g, data["P"], data["w8"], True, 1)
    good = np.full((PERIODS, B), 0.5 * H)
    clean = fly(g, data["x13"], data["u"], good)
    tau = good.copy()
    tau[:, 5] = np.nan
    tau[:, 66] = -0.01
    out = fly(g, data["x13"], data["u"], tau)
    others = [b for b in range(B) if b not in (5, 66)]
    for p in range(PERIODS):
        assert out[p]["st"][5] == ok.PLANT_BAD_TAU and out[p]["st"][66] == ok.PLANT_BAD_TAU
        assert not out[p]["st"][others].any()
        assert not out[p]["line"][[5, 66]].any() and not out[p]["ua"][[5, 66]].any()        # still fresh, flying zero
        for k in ("x", "line", "ua"):
            np.testing.assert_array_equal(out[p][k][others], clean[p][k][others], err_msg=f"{k}, period {p}")


# ---- (f) non-finite kite -------------------------------------------------------
def test_a_non_finite_kite_is_frozen_and_its_line_goes_on(g, data):
    clean = fly(g, data["x13"], data["u"], data["tau_b"])
    x = data["x13"].copy()
    x[10, 0], x[69, 11] = np.nan, np.inf          # one per block, non-finite on entry
    x[3, 0] = 1e160                               # finite on entry, overflows in the first substep
    frozen = [3, 10, 69]
    out = fly(g, x, data["u"], data["tau_b"])
    others = [b for b in range(B) if b not in frozen]
    for p in range(PERIODS):
        for b in frozen:
            assert np.array_equal(out[p]["x"][b], x[b], equal_nan=True), (p, b)
            assert out[p]["st"][b] & ok.PLANT_NAN, (p, b)
        assert not (out[p]["st"][others] & ok.PLANT_NAN).any()
        np.testing.assert_array_equal(out[p]["line"], clean[p]["line"])             # the queue does not look at the state
        np.testing.assert_array_equal(out[p]["ua"], clean[p]["ua"])
        np.testing.assert_array_equal(out[p]["x"][others], clean[p]["x"][others])


# ---- (h) host vs device --------------------------------------------------------
def test_device_and_host_entry_points_agree(g, data):
    set_plant(g, data["P"], data["w8"], True, 2)
    want = fly(g, data["x13"], data["u"], data["tau_b"], by_substep=True, send=lambda p: p != 3)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        x = torch.from_numpy(data["x13"].copy()).cuda()
        line = torch.zeros((B, ok.DELAY_NLINE), dtype=torch.float64, device="cuda")
        ua = torch.full((B, 4), 7.0, dtype=torch.float64, device="cuda")
        st = torch.full((B,), 77, dtype=torch.int32, device="cuda")              # written, not OR-ed
        t = 0.0
        for p in range(PERIODS):
            u = torch.from_numpy(data["u"][p].copy()).cuda()
            tau = torch.from_numpy(data["tau_b"][p].copy()).cuda()
            g.plant_step_delayed_device(x.data_ptr(), u.data_ptr() if p != 3 else 0, tau.data_ptr() if p != 3 else 0,
                                        line.data_ptr(), t, H, STEPS, SUB, ua.data_ptr(), st.data_ptr())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(x.cpu().numpy(), want[p]["x"], err_msg=f"period {p}")
            np.testing.assert_array_equal(line.cpu().numpy(), want[p]["line"], err_msg=f"period {p}")
            np.testing.assert_array_equal(ua.cpu().numpy(), want[p]["ua"], err_msg=f"period {p}")
            np.testing.assert_array_equal(st.cpu().numpy(), want[p]["st"], err_msg=f"period {p}")
            t += DT
        # u_applied and the status are optional
        g.plant_step_delayed_device(x.data_ptr(), 0, 0, line.data_ptr(), t, H, STEPS, SUB)
        torch.cuda.synchronize()
        assert torch.isfinite(x).all()
    finally:
        g.use_own_stream()


# ---- (i) batch position --------------------------------------------------------
def test_a_kites_row_does_not_depend_on_the_batch(g, data):
    set_plant(g, data["P"], data["w8"], True, 2)
    want = fly(g, data["x13"], data["u"], data["tau_b"], by_substep=True)
    perm = np.random.default_rng(3).permutation(B)
    set_plant(g, data["P"][perm], data["w8"][perm], True, 2)
    got = fly(g, data["x13"][perm], data["u"][:, perm], data["tau_b"][:, perm], by_substep=True)
    for p in range(PERIODS):
        for k in ("x", "line", "ua", "st"):
            np.testing.assert_array_equal(got[p][k], want[p][k][perm], err_msg=f"{k}, period {p}")
    for nk in (1, 3):
        sel = np.array([6, 41, 69][:nk])                                    # the kite beyond the depth among them
        c = ok.BatchNMPC(ok.load_properties(), ok.default_config(), nk)
        try:
            set_plant(c, data["P"][sel], data["w8"][sel], True, 2)
            got = fly(c, data["x13"][sel], data["u"][:, sel], data["tau_b"][:, sel], by_substep=True)
        finally:
            c.close()
        for p in range(PERIODS):
            for k in ("x", "line", "ua", "st"):
                np.testing.assert_array_equal(got[p][k], want[p][k][sel], err_msg=f"B = {nk}: {k}, period {p}")


# ---- (j) bad arguments ---------------------------------------------------------
def test_bad_arguments_are_refused_and_change_nothing(g, data):
    L = ok.lib()
    x = np.ascontiguousarray(data["x13"]).copy()
    u = np.ascontiguousarray(data["u"][0]).copy()
    tau = np.full(B, 0.5 * H)
    line = np.zeros((B, ok.DELAY_NLINE))
    line[:, nmpc.DELAY_U_FORCE] = 0.11
    ua = np.zeros((B, 4))
    st = np.zeros(B, dtype=np.int32)
    x_was, line_was = x.copy(), line.copy()
    ok_args = dict(x=nmpc._p(x), u=nmpc._p(u), tau=nmpc._p(tau), line=nmpc._p(line), t0=0.0, h=H, steps=STEPS, substeps=SUB)
    cases = [dict(line=None), dict(tau=None), dict(x=None), dict(h=0.0), dict(h=-H), dict(h=np.nan), dict(h=np.inf),
             dict(steps=0), dict(substeps=0), dict(t0=np.nan), dict(t0=np.inf), dict(steps=1 << 20, substeps=1 << 5)]
    for kw in cases:
        a = dict(ok_args)
        a.update(kw)
        rc = L.kite_nmpc_plant_step_delayed(g._h, a["x"], a["u"], a["tau"], a["line"], nmpc._p(ua), a["t0"], a["h"],
                                            a["steps"], a["substeps"], st.ctypes.data_as(nmpc._IP))
        assert rc == nmpc.KITE_EINVAL, kw
        np.testing.assert_array_equal(x, x_was)
        np.testing.assert_array_equal(line, line_was)
        assert not ua.any() and not st.any()
    assert L.kite_nmpc_plant_step_delayed(None, *[ok_args[k] for k in ("x", "u", "tau", "line")], nmpc._p(ua), 0.0, H,
                                          STEPS, SUB, None) == nmpc.KITE_EINVAL
    # the device entry: the same checks, nothing launched
    dx, dl = torch.from_numpy(x_was.copy()).cuda(), torch.from_numpy(line_was.copy()).cuda()
    du, dt_ = torch.from_numpy(u).cuda(), torch.from_numpy(tau).cuda()
    for kw in (dict(line=0), dict(tau=0), dict(x=0), dict(h=0.0), dict(steps=0), dict(substeps=0), dict(t0=np.nan)):
        a = dict(x=dx.data_ptr(), u=du.data_ptr(), tau=dt_.data_ptr(), line=dl.data_ptr(), t0=0.0, h=H, steps=STEPS,
                 substeps=SUB)
        a.update(kw)
        with pytest.raises(ok.KiteNmpcError) as e:
            g.plant_step_delayed_device(a["x"], a["u"], a["tau"], a["line"], a["t0"], a["h"], a["steps"], a["substeps"])
        assert e.value.code == nmpc.KITE_EINVAL, kw
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dx.cpu().numpy(), x_was)
    np.testing.assert_array_equal(dl.cpu().numpy(), line_was)
    # no command: tau is not needed; and the valid call still works
    got = g.plant_step_delayed(x, None, None, line, 0.0, H, STEPS, SUB)
    assert not got[3].any() and np.all(got[2][:, 0] == 0.11)


# ---- (k) FleetLoop against the model on the host --------------------------------
class RefDelayedPlant:
    """A plant for FleetLoop that knows nothing of the delayed kernel: the line
    is tests/delay_ref.py on the host, the flight the undelayed
    plant_step(steps=1) per plant step.  The latencies are those an
    ActuationDelay of the same seed draws."""

    def __init__(self, ctx, nk, h, steps, substeps, mean, deviation, seed):
        self.ctx, self.h, self.steps, self.substeps = ctx, h, steps, substeps
        self.taus = ActuationDelay(nk, mean, deviation, seed=seed, device="cuda")
        self.fleet = dr.Fleet(nk)
        self.dropped = 0

    def advance(self, x13, u0, t0, status):
        tau = self.taus.draw().cpu().numpy()
        u_steps, _, _, bits = self.fleet.call(u0.cpu().numpy(), tau, t0, self.h, self.steps, self.substeps)
        x, st = x13.cpu().numpy(), bits.copy()
        hs = self.h / self.substeps
        for j in range(self.steps):
            x, s = self.ctx.plant_step(x, u_steps[j], t0 + float(j * self.substeps) * hs, self.h, 1, self.substeps)
            st |= s
        x13.copy_(torch.from_numpy(x))
        status.copy_(torch.from_numpy(st))
        self.dropped += int((bits & dr.CMD_DROPPED != 0).sum())


@pytest.mark.parametrize("deviation", [0.0, 0.02])
def test_fleet_loop_with_a_delayed_plant_equals_the_model(deviation):
    from bench import synthetic_x0
    nk, Nh, periods = 16, 20, 6
    cfg = ok.default_config(N=Nh)
    h, psteps, sub = cfg.dt / 2, 2, 5
    mean = 2 * cfg.dt
    rng = np.random.default_rng(29)
    P = ok.perturb_params(ffi.load_params(), nk, 0.1, seed=29)
    W0 = rng.uniform(-0.3, 0.3, (nk, 3))
    a = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    b = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    try:
        for c in (a, b):
            c.plant_set_params(P)
            c.plant_set_wind(W0)
            c.set_stream(torch.cuda.current_stream().cuda_stream)
        x_init = torch.from_numpy(synthetic_x0(nk, 0, a)).cuda()
        delay = ActuationDelay(nk, mean, deviation, seed=17, device="cuda")
        la = FleetLoop(GpuStepper(a), x_init, Nh, cfg.dt, plant=GpuPlant(a, h, psteps, sub, delay=delay),
                       scorer=EpisodeScore(nk, device="cuda"))
        ref_plant = RefDelayedPlant(b, nk, h, psteps, sub, mean, deviation, seed=17)
        lb = FleetLoop(GpuStepper(b), x_init, Nh, cfg.dt, plant=ref_plant, scorer=EpisodeScore(nk, device="cuda"))
        assert la.delay is delay and lb.delay is None
        for s in range(periods):
            la.step()
            lb.step()
            np.testing.assert_array_equal(delay.tau.cpu().numpy(), ref_plant.taus.tau.cpu().numpy())
            for name in ("u0", "xp", "x0", "plant_status"):
                np.testing.assert_array_equal(getattr(la, name).cpu().numpy(), getattr(lb, name).cpu().numpy(),
                                              err_msg=f"{name}, period {s}")
            np.testing.assert_array_equal(la.scorer.acc.cpu().numpy(), lb.scorer.acc.cpu().numpy(), err_msg=f"acc, period {s}")
        assert torch.isfinite(la.xp).all()
        # the delay is felt: the first two periods fly the fresh line's zero control
        assert not torch.equal(delay.u_applied, la.u0)
        # restart: fresh lines, the generator back at its seed, the same flight again
        first = la.xp.clone()
        la.restart()
        assert not delay.line.any() and not delay.u_applied.any()
        for s in range(periods):
            la.step()
        assert torch.equal(la.xp, first)
    finally:
        a.close()
        b.close()


# ---- (l) recorder rule -----------------------------------------------------------
def test_a_recorder_is_refused_where_the_control_is_not_constant_over_a_period():
    nk, Nh = 4, 20
    cfg = ok.default_config(N=Nh)
    c = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    try:
        from bench import synthetic_x0
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        x_init = torch.from_numpy(synthetic_x0(nk, 0, c)).cuda()

        def loop(mean, deviation):
            d = ActuationDelay(nk, mean, deviation, device="cuda")
            return FleetLoop(GpuStepper(c), x_init, Nh, cfg.dt, plant=GpuPlant(c, cfg.dt / 2, 2, 5, delay=d),
                             recorder=FlightRecorder(nk, 3, device="cuda"))
        with pytest.raises(ValueError, match="deviation"):
            loop(2 * cfg.dt, 0.005)
        with pytest.raises(ValueError, match="whole number"):
            loop(0.02, 0.0)
        # accepted: the log holds what flew, which is not what was commanded
        lp = loop(cfg.dt, 0.0)
        for _ in range(3):
            lp.step()
        U = lp.recorder.U.cpu().numpy()
        assert lp.recorder.nu == 3 and not U[:, 0].any() and U[:, 1].any()        # period 0 flew the fresh line's zero
        np.testing.assert_array_equal(U[:, 2], lp.plant.delay.u_applied[:, :3].cpu().numpy())
    finally:
        c.close()


# ---- (m) driver --------------------------------------------------------------------
def test_driver_flies_the_delayed_plant(tmp_path):
    nk, S, K = 4, 6, 3
    x13 = ffi.synthetic_states(nk, offset=980)
    np.savetxt(tmp_path / "x0.csv", x13, delimiter=",", fmt="%.17g")
    out = subprocess.run([DRIVER, "--params", PARAMS, "--batch", str(nk), "--steps", str(S), "--x0", str(tmp_path / "x0.csv"),
                          "--ctrl-every", str(K), "--sim-dt", "0.02", "--delay", "0.1", "--trace", str(nk),
                          "--plant-delay", "0.1"], check=True, capture_output=True, text=True).stdout
    recs = [json.loads(l) for l in out.strip().splitlines()]
    diag = {(r["step"], r["kite"]): r for r in recs if r["type"] == "mpc_diagnostic"}
    summary = [r for r in recs if r["type"] == "step"]
    assert len(summary) == S and all("cmd_dropped" in r and "plant_nan" not in r for r in summary)
    c = ok.BatchNMPC(ok.load_properties(), ok.default_config(delay=0.1, delay_steps=16), nk)
    try:
        plant, t, traj = x13.copy(), 0.0, None
        line = np.zeros((nk, ok.DELAY_NLINE))
        st = np.zeros(nk, dtype=np.int32)
        theta = c.closest_point(plant[:, 6:9], np.zeros(nk))
        for s in range(S):
            x0 = np.zeros((nk, 15))
            x0[:, :13] = plant
            x0[:, 13] = theta if s == 0 else traj[:, 1, 13]
            x0[:, 14] = 0.0 if s == 0 else traj[:, 1, 14]
            r = c.step(x0)
            traj = r["traj"]
            assert summary[s]["cmd_dropped"] == int(((st & ok.PLANT_CMD_DROPPED) != 0).sum())
            for b in range(nk):
                np.testing.assert_array_equal(np.array(diag[(s, b)]["x"]), plant[b], err_msg=f"step {s} kite {b}")
                np.testing.assert_array_equal(np.array(diag[(s, b)]["u"]), r["u0"][b])
            u4 = r["u0"].copy()
            u4[:, 3] = 0.0
            plant, line, ua, st = c.plant_step_delayed(plant, u4, np.full(nk, 0.1), line, t, 0.02, K, 4)
            if s < 1:
                assert not ua.any()                   # 0.1 s: nothing has arrived in the first period
            for _ in range(K):
                t += 0.02
    finally:
        c.close()
