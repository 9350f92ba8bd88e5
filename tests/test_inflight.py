"""The in-flight schedule and the queue-aware delay compensation
(kite_nmpc_set_inflight[_device], _get_inflight; k_inflight and prologue_kite in
openkite_amd/csrc/rti_kernels.hip; BatchNMPC.set_inflight, FleetLoop(delay_comp=),
nmpf_driver --delay-comp).

B = 70, N = 20, delay = 0.1, delay_steps = 16: one cold step, then a warm step on
a perturbed state.  The schedule rows are compared bit for bit with
delay_rule_ref.inflight_row; the predicted state traj[:, 0, :13] with the
oracle's RK4 composed over delay_rule_ref.segments to 1e-12 relative, the bar
test_gpu_parity.test_predict_vs_oracle holds for this integrator against this
oracle function; everything that must not change is compared bitwise against a
context that never received a schedule.

Measured on the MI355X (max over the kites compared, relative to max(1, |x|)):
guard (no schedule, one piece) 8.2e-16; queue-aware (1 to 5 pieces) 1.2e-15.
"""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import ActuationDelay, FleetLoop, GpuPlant, GpuStepper
from oracle import ffi

import delay_ref as dr
import delay_rule_ref as rr

pytestmark = pytest.mark.gpu

B, N, D, DS = 70, 20, 0.1, 16
T0 = 0.015625                   # 2^-6: T0 + D is exact, so an arrival can sit exactly at the window's end
TOL = 1e-12
NPAT = 14
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "openkite_amd", "bin", "nmpf_driver")
PARAMS = os.path.join(REPO, "data", "umx_radian.yaml")
KEYS = ("u0", "traj", "ctrl", "status")


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def config(**kw):
    return ok.default_config(N=N, delay=D, delay_steps=DS, **kw)


def states(nk, offset):
    cv = ffi.cfg_vector(ffi.node_config())
    x0 = np.zeros((nk, 15))
    x0[:, :13] = ffi.synthetic_states(nk, offset=offset)
    for b in range(nk):
        x0[b, 13] = ffi.closest_point(cv, x0[b, 6:9])
    return x0


def crafted_lines(nk, rng):
    """(nk, 32) lines seen at T0, pattern b % NPAT (see the comments), and the
    patterns whose schedule row is invalid."""
    def cmd():
        return [rng.uniform(0.1, 0.15), rng.uniform(-0.12, 0.12), rng.uniform(-0.12, 0.12), rng.uniform(-1, 1)]

    line = np.zeros((nk, dr.NLINE))
    for b in range(nk):
        L, pat = line[b], b % NPAT
        L[dr.U_FORCE:dr.U_FORCE + 4] = cmd()
        arr = []
        if pat == 0:
            arr = []                                          # an empty FIFO
        elif pat == 1:
            arr = [T0 - 0.02]                                 # arrived before t0: flies from the start
        elif pat == 2:
            arr = [T0 + 0.03]                                 # inside the window
        elif pat == 3:
            arr = [T0 + D]                                    # exactly at the end: no switch
        elif pat == 4:
            arr = [T0 + 0.17]                                 # beyond
        elif pat == 5:
            arr = [T0 + 0.02, T0 + 0.05, T0 + 0.05, T0 + 0.08]   # four, two at the same instant
        elif pat == 6:
            arr = [T0 + 0.06, T0 + 0.03, T0 + 0.07]           # decreasing: the running maximum
        elif pat == 7:
            arr = [T0 + 0.04, T0 + 0.05]                      # count NaN: read as 0, the slots are ignored
        elif pat == 8:
            arr = [T0 + 0.01, T0 + 0.0225, T0 + 0.05, np.nextafter(T0 + D, 0.0)]   # count 7: read as 4; five pieces
        elif pat == 9:
            arr = [T0 + 0.02, np.nan]                         # NaN arrival time
        elif pat == 10:
            arr = [T0 + 0.02, T0 + 0.04]                      # NaN in a pending command (below)
        elif pat == 11:
            arr = [T0 + 0.02]                                 # inf in the control in force (below)
        elif pat == 12:
            arr = [T0 + 0.02, T0 + 0.04]                      # NaN in 4th controls only: ignored
        elif pat == 13:
            arr = [T0 + 0.02]                                 # NaN beyond the count: ignored
        L[dr.COUNT] = len(arr)
        for s, ta in enumerate(arr):
            L[dr.T_ARR + s] = ta
            L[dr.U + 4 * s:dr.U + 4 * s + 4] = cmd()
        if pat == 7:
            L[dr.COUNT] = np.nan
        elif pat == 8:
            L[dr.COUNT] = 7.0
        elif pat == 10:
            L[dr.U + 4 + 1] = np.nan
        elif pat == 11:
            L[dr.U_FORCE + 2] = np.inf
        elif pat == 12:
            L[dr.U_FORCE + 3] = L[dr.U + 3] = L[dr.U + 7] = np.nan
        elif pat == 13:
            L[dr.T_ARR + 2] = L[dr.U + 9] = np.nan
        L[dr.T_PREV], L[dr.HAS_PREV], L[rr.RULE] = 123.0, 1.0, float(b % 2)      # not the schedule's business
    return line, (9, 10, 11)


def two_steps(nk, x0, x1, line=None, t0=T0, wind=None, params=None, device=False, cfg_kw=None, then=None):
    """A context's cold step on x0, the schedule (if any), the warm step on x1;
    returns (cold, warm, schedule rows or None).  ``then(ctx, warm)`` runs before it closes."""
    c = ok.BatchNMPC(ok.load_properties(), config(**(cfg_kw or {})), nk)
    try:
        if wind is not None:
            c.set_wind(wind)
        if params is not None:
            c.set_params(params)
        cold = c.step(x0)
        sched = None
        if line is not None:
            if device:
                d = torch.from_numpy(line.copy()).cuda()
                torch.cuda.synchronize()
                c.set_inflight_device(d.data_ptr(), t0)
                c.synchronize()
            else:
                c.set_inflight(line, t0)
            sched = c.get_inflight()
        warm = c.step(x1)
        if then is not None:
            then(c, warm)
        return cold, warm, sched
    finally:
        c.close()


def same_step(a, b, rows=slice(None), msg=""):
    for k in KEYS:
        np.testing.assert_array_equal(a[k][rows], b[k][rows], err_msg=f"{k} {msg}")
    np.testing.assert_array_equal(a["diag"][rows, :5], b["diag"][rows, :5], err_msg=f"diag {msg}")     # [5]: wall time


@pytest.fixture(scope="module")
def base(kp):
    """The no-schedule context's two steps and the crafted lines (shared, read-only)."""
    rng = np.random.default_rng(1618)
    x0 = states(B, 7000)
    cold, _, _ = two_steps(B, x0, x0)               # the plan the warm state is taken from
    x1 = x0.copy()
    x1[:, :13] = cold["traj"][:, 1, :13] + rng.normal(scale=0.01, size=(B, 13))
    x1[:, 13:] = cold["traj"][:, 1, 13:]
    cold, warm, _ = two_steps(B, x0, x1)
    line, bad = crafted_lines(B, rng)
    for a in (x0, x1, line):
        a.setflags(write=False)
    return dict(x0=x0, x1=x1, cold=cold, warm=warm, line=line, bad=bad, u_prev=cold["ctrl"][:, 0].copy())


def oracle_window(kp, x15, pieces):
    x = np.array(x15, dtype=np.float64)
    for u3, h, n in pieces:
        x = ffi.rk4(kp, x, np.array([u3[0], u3[1], u3[2], 0.0]), h, n)
    return x[:13]


def test_guard_no_schedule_is_the_oracles_rk4(base, kp):
    st = base["warm"]["status"]
    assert not (st & nmpc.ST_MIN_SPEED).any() and not (st & (nmpc.ST_RESTART | nmpc.ST_BAD_INFLIGHT)).any()
    worst = 0.0
    for b in range(B):
        up = np.array([*base["u_prev"][b, :3], 0.0])
        worst = max(worst, rel(base["warm"]["traj"][b, 0, :13], ffi.rk4(kp, base["x1"][b], up, D / DS, DS)[:13]))
    print(f"guard: max rel {worst:.3e}")
    assert worst < TOL


@pytest.mark.parametrize("device", [False, True])
def test_crafted_lines(base, kp, device):
    line = base["line"]
    cold, warm, sched = two_steps(B, base["x0"], base["x1"], line=line, device=device)
    want = rr.inflight_rows(line, T0)
    np.testing.assert_array_equal(sched, want)
    pat = np.arange(B) % NPAT
    invalid = np.isin(pat, base["bad"])
    np.testing.assert_array_equal(want[:, 0] == -1.0, invalid)
    assert want[pat == 3][:, 1].tolist() == [D] * int((pat == 3).sum())           # exactly at the end
    assert set(want[pat == 7][:, 0]) == {0.0} and set(want[pat == 8][:, 0]) == {4.0}
    assert np.all(want[pat == 6][:, 1] == want[pat == 6][:, 2])                     # the running maximum
    same_step(cold, base["cold"], msg="(cold step)")
    # invalid rows: the no-schedule prediction and the flag; nobody else is flagged
    np.testing.assert_array_equal((warm["status"] & nmpc.ST_BAD_INFLIGHT) != 0, invalid)
    for k in ("u0", "traj", "ctrl"):
        np.testing.assert_array_equal(warm[k][invalid], base["warm"][k][invalid], err_msg=k)
    np.testing.assert_array_equal(warm["status"][invalid] & ~np.int32(nmpc.ST_BAD_INFLIGHT), base["warm"]["status"][invalid])
    # valid rows: the oracle's RK4 composed over the pieces
    assert not (warm["status"] & (nmpc.ST_MIN_SPEED | nmpc.ST_RESTART)).any()
    worst, npieces = 0.0, set()
    for b in np.flatnonzero(~invalid):
        pieces = rr.segments(want[b], D, DS)
        npieces.add(len(pieces))
        worst = max(worst, rel(warm["traj"][b, 0, :13], oracle_window(kp, base["x1"][b], pieces)))
    print(f"queue-aware: max rel {worst:.3e} over pieces {sorted(npieces)}")
    assert npieces >= {1, 2, 4, 5} and worst < TOL
    # the schedule is felt where a command in flight differs from the previous u(t0)
    assert np.abs(warm["traj"][~invalid, 0, :13] - base["warm"]["traj"][~invalid, 0, :13]).max() > 1e-6


def empty_lines(u_prev):
    line = np.zeros((u_prev.shape[0], dr.NLINE))
    line[:, dr.U_FORCE:dr.U_FORCE + 3] = u_prev[:, :3]
    return line


def test_an_empty_fifo_under_the_previous_control_is_todays_step(base):
    _, warm, sched = two_steps(B, base["x0"], base["x1"], line=empty_lines(base["u_prev"]))
    assert not sched[:, 0].any()
    same_step(warm, base["warm"])


def test_the_same_with_per_kite_rows_equal_to_the_creation_row(base):
    rows = np.tile(ok.load_properties().as_array(), (B, 1))
    _, ref, _ = two_steps(B, base["x0"], base["x1"], params=rows)
    _, warm, _ = two_steps(B, base["x0"], base["x1"], params=rows, line=empty_lines(base["u_prev"]))
    same_step(warm, ref)


def test_the_same_with_a_controller_wind(base):
    wind = np.random.default_rng(5).uniform(-1.0, 1.0, (B, 3))
    cold, ref, _ = two_steps(B, base["x0"], base["x1"], wind=wind)
    assert np.abs(ref["traj"][:, 0, :13] - base["warm"]["traj"][:, 0, :13]).max() > 1e-6        # the wind is felt
    _, warm, _ = two_steps(B, base["x0"], base["x1"], wind=wind, line=empty_lines(cold["ctrl"][:, 0]))
    same_step(warm, ref)
    # and under the wind a schedule moves the prediction
    _, moved, _ = two_steps(B, base["x0"], base["x1"], wind=wind, line=base["line"])
    assert np.abs(moved["traj"][:, 0, :13] - ref["traj"][:, 0, :13]).max() > 1e-6


def test_clearing_the_schedule_restores_todays_step_and_reset_keeps_it(base):
    c = ok.BatchNMPC(ok.load_properties(), config(), B)
    try:
        c.step(base["x0"])
        c.set_inflight(base["line"], T0)
        c.set_inflight(None)
        with pytest.raises(ok.KiteNmpcError) as e:
            c.get_inflight()
        assert e.value.code == nmpc.KITE_ESTATE
        same_step(c.step(base["x1"]), base["warm"])
        # reset keeps a schedule; the cold step ignores it; the next warm step uses it
        c.set_inflight(base["line"], T0)
        c.reset()
        same_step(c.step(base["x0"]), base["cold"])
        np.testing.assert_array_equal(c.get_inflight(), rr.inflight_rows(base["line"], T0))
        warm = c.step(base["x1"])
        assert (warm["status"] & nmpc.ST_BAD_INFLIGHT).any()
        with pytest.raises(ok.KiteNmpcError) as e:
            c.set_inflight(base["line"], np.nan)
        assert e.value.code == nmpc.KITE_EINVAL
    finally:
        c.close()


def test_no_delay_no_schedule():
    c = ok.BatchNMPC(ok.load_properties(), ok.default_config(N=N), 3)
    try:
        line = np.zeros((3, dr.NLINE))
        with pytest.raises(ok.KiteNmpcError) as e:
            c.set_inflight(line, 0.0)
        assert e.value.code == nmpc.KITE_ESTATE
        d = torch.zeros((3, dr.NLINE), dtype=torch.float64, device="cuda")
        with pytest.raises(ok.KiteNmpcError) as e:
            c.set_inflight_device(d.data_ptr(), 0.0)
        assert e.value.code == nmpc.KITE_ESTATE
        with pytest.raises(ok.KiteNmpcError) as e:
            c.get_inflight()
        assert e.value.code == nmpc.KITE_ESTATE
        c.set_inflight(None)                        # switching off what is off is fine
        with pytest.raises(ValueError):
            c.set_inflight(np.zeros((3, 31)))
    finally:
        c.close()


@pytest.mark.parametrize("nk", [1, 3])
def test_small_batches(base, nk):
    sel = np.array([5, 36, 9][:nk])                  # four pending, the decreasing arrivals, an invalid row
    cold, warm, sched = two_steps(nk, base["x0"][sel], base["x1"][sel], line=base["line"][sel])
    np.testing.assert_array_equal(sched, rr.inflight_rows(base["line"][sel], T0))
    _, full, _ = two_steps(B, base["x0"], base["x1"], line=base["line"])
    np.testing.assert_array_equal(warm["traj"][:, 0], full["traj"][sel, 0])
    np.testing.assert_array_equal(warm["status"] & nmpc.ST_BAD_INFLIGHT, full["status"][sel] & nmpc.ST_BAD_INFLIGHT)


# ---- closed loop ---------------------------------------------------------------------
def fleet(nk, cfg, mean, deviation, rule, comp):
    from bench import synthetic_x0
    c = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    x_init = torch.from_numpy(synthetic_x0(nk, 0, c)).cuda()
    delay = ActuationDelay(nk, mean, deviation, seed=23, device="cuda", rule=rule)
    loop = FleetLoop(GpuStepper(c), x_init, N, cfg.dt, plant=GpuPlant(c, cfg.dt / 2, 2, 5, delay=delay), delay_comp=comp)
    return c, loop


@pytest.mark.parametrize("deviation", [0.0, 0.02])
def test_fleet_loop_queue_equals_the_schedule_built_on_the_host(deviation):
    nk, periods = 8, 6
    cfg = config()
    a, la = fleet(nk, cfg, 2 * cfg.dt, deviation, "transport", "queue")
    b, lb = fleet(nk, cfg, 2 * cfg.dt, deviation, "transport", "last")      # this loop hands nothing over itself
    try:
        pending = 0
        for s in range(periods):
            la.step()
            line = lb.delay.line.cpu().numpy()
            b.set_inflight(line, lb.t)                                      # the host entry
            np.testing.assert_array_equal(b.get_inflight(), rr.inflight_rows(line, lb.t))
            np.testing.assert_array_equal(a.get_inflight(), b.get_inflight(), err_msg=f"period {s}")
            pending = max(pending, int(line[:, dr.COUNT].max()))
            lb.step()
            for name in ("u0", "xp", "status"):
                np.testing.assert_array_equal(getattr(la, name).cpu().numpy(), getattr(lb, name).cpu().numpy(),
                                              err_msg=f"{name}, period {s}")
        assert pending >= 2 and torch.isfinite(la.xp).all()                # two commands were in flight
        assert not (la.status.cpu().numpy() & nmpc.ST_BAD_INFLIGHT).any()
    finally:
        a.close()
        b.close()


def test_at_one_period_queue_and_last_are_the_same_loop():
    nk, periods = 8, 6
    cfg = ok.default_config(N=N, delay=0.05, delay_steps=DS)
    a, la = fleet(nk, cfg, cfg.dt, 0.0, "transport", "queue")
    b, lb = fleet(nk, cfg, cfg.dt, 0.0, "transport", "last")
    try:
        for s in range(periods):
            la.step()
            lb.step()
            np.testing.assert_array_equal(la.u0.cpu().numpy(), lb.u0.cpu().numpy(), err_msg=f"period {s}")
        sched = a.get_inflight()
        assert np.all(sched[:, 0] == 1.0) and not sched[:, 1].any()        # one command, from the window's start
    finally:
        a.close()
        b.close()


# ---- driver ----------------------------------------------------------------------------
def test_driver_flies_the_queue_aware_compensation(tmp_path):
    nk, S, K = 4, 6, 3
    x13 = ffi.synthetic_states(nk, offset=990)
    np.savetxt(tmp_path / "x0.csv", x13, delimiter=",", fmt="%.17g")
    out = subprocess.run([DRIVER, "--params", PARAMS, "--batch", str(nk), "--steps", str(S), "--x0", str(tmp_path / "x0.csv"),
                          "--ctrl-every", str(K), "--sim-dt", "0.02", "--delay", "0.1", "--trace", str(nk),
                          "--plant-delay", "0.1", "--plant-delay-rule", "transport", "--delay-comp", "queue"],
                         check=True, capture_output=True, text=True).stdout
    recs = [json.loads(l) for l in out.strip().splitlines()]
    diag = {(r["step"], r["kite"]): r for r in recs if r["type"] == "mpc_diagnostic"}
    c = ok.BatchNMPC(ok.load_properties(), ok.default_config(delay=0.1, delay_steps=16), nk)
    try:
        plant, t, traj = x13.copy(), 0.0, None
        line = np.zeros((nk, ok.DELAY_NLINE))
        line[:, nmpc.DELAY_RULE] = nmpc.DELAY_RULE_TRANSPORT
        theta = c.closest_point(plant[:, 6:9], np.zeros(nk))
        for s in range(S):
            x0 = np.zeros((nk, 15))
            x0[:, :13] = plant
            x0[:, 13] = theta if s == 0 else traj[:, 1, 13]
            x0[:, 14] = 0.0 if s == 0 else traj[:, 1, 14]
            c.set_inflight(line, t)
            r = c.step(x0)
            traj = r["traj"]
            for b in range(nk):
                np.testing.assert_array_equal(np.array(diag[(s, b)]["x"]), plant[b], err_msg=f"step {s} kite {b}")
                np.testing.assert_array_equal(np.array(diag[(s, b)]["u"]), r["u0"][b], err_msg=f"step {s} kite {b}")
            u4 = r["u0"].copy()
            u4[:, 3] = 0.0
            plant, line, ua, st = c.plant_step_delayed(plant, u4, np.full(nk, 0.1), line, t, 0.02, K, 4)
            assert not (st & ok.PLANT_CMD_DROPPED).any()
            for _ in range(K):
                t += 0.02
        # the flags are refused where they make no sense
        assert subprocess.run([DRIVER, "--params", PARAMS, "--batch", "1", "--steps", "1", "--delay-comp", "queue"],
                              capture_output=True).returncode == 2
        assert subprocess.run([DRIVER, "--params", PARAMS, "--batch", "1", "--steps", "1", "--plant-delay", "0.1",
                               "--plant-delay-rule", "fifo"], capture_output=True).returncode == 2
    finally:
        c.close()
