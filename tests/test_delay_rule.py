"""The command line's second arrival rule (slot KITE_DELAY_RULE of the line;
delay_send in openkite_amd/csrc/delay_line.hpp, k_plant_delay;
fleet.ActuationDelay(rule=)) and the models of tests/delay_rule_ref.py.

CPU: the models against the semantics they restate.  GPU (as
test_plant_delay.py: bit for bit, B = 70, 3 steps x 2 substeps, 8 periods):
lines alternate their rule by kite index within one launch; the expected line,
u_applied and status bits are the model's, the expected state is composed from
the undelayed kite_nmpc_plant_step under the controls the model says are in
force.
"""
import math

import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import ActuationDelay

import delay_ref as dr
import delay_rule_ref as rr

B = 70
H, STEPS, SUB, PERIODS = 0.02, 3, 2, 8
HS, DT = H / SUB, STEPS * H
# on the tick, inside a step, across a step, one period, the node's two, across periods, beyond the depth
TAU_CYCLE = np.array([0.0, 0.5 * H, 1.3 * H, DT, 2 * DT, 2.4 * DT, 4.7 * DT])
RULES = (np.arange(B) % 2).astype(np.float64)             # even kites sequential, odd kites transport


# ---- CPU: the models -----------------------------------------------------------
def test_the_constants_agree():
    assert (nmpc.DELAY_RULE, nmpc.DELAY_RULE_SEQUENTIAL, nmpc.DELAY_RULE_TRANSPORT) == (3, 0, 1)
    assert (rr.RULE, rr.RULE_SEQUENTIAL, rr.RULE_TRANSPORT) == (3, 0.0, 1.0)
    assert nmpc.INFLIGHT_N == rr.INFLIGHT_N == 24 and nmpc.ST_BAD_INFLIGHT == 128
    L = ok.lib()
    assert L.kite_nmpc_api_version() == 7
    for name in ("kite_nmpc_set_inflight", "kite_nmpc_set_inflight_device", "kite_nmpc_get_inflight"):
        assert hasattr(L, name) and name in nmpc._SIGNATURES


def random_calls(rng, nk, periods):
    calls, t = [], 0.0
    for p in range(periods):
        send = rng.uniform() < 0.8
        tau = rng.choice([0.0, 0.3 * DT, DT, 2 * DT, 4.7 * DT, -1.0, np.nan], size=nk)
        calls.append(dict(u_cmd=rng.uniform(-0.2, 0.2, (nk, 4)) if send else None, tau=tau, t0=t, h=H, steps=STEPS,
                          substeps=SUB))
        t += DT
    return calls


@pytest.mark.parametrize("slot", [0.0, np.nan, 2.0, -1.0, 0.999999])
def test_any_slot_value_but_one_is_the_sequential_rule(slot):
    nk = 5
    calls = random_calls(np.random.default_rng(11), nk, 30)
    a, b = dr.Fleet(nk), rr.Fleet(nk, np.full(nk, slot))
    for c in calls:
        ra = a.call(c["u_cmd"], c["tau"], c["t0"], c["h"], c["steps"], c["substeps"])
        rb = b.call(c["u_cmd"], c["tau"], c["t0"], c["h"], c["steps"], c["substeps"])
        rows = rb[1].copy()
        assert np.array_equal(rows[:, rr.RULE], np.full(nk, slot), equal_nan=True)
        rows[:, rr.RULE] = 0.0
        np.testing.assert_array_equal(rows, ra[1])
        for x, y in zip((ra[0], ra[2], ra[3]), (rb[0], rb[2], rb[3])):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("jitter", [0.0, 0.1])
def test_transport_at_two_periods_drops_nothing(jitter):
    rng = np.random.default_rng(4)
    nk = 6
    f, seq = rr.Fleet(nk, np.ones(nk)), rr.Fleet(nk, np.zeros(nk))
    t, dropped_seq = 0.0, 0
    for p in range(40):
        tau = 2 * DT * (1.0 + jitter * rng.uniform(-1.0, 1.0, nk))
        u = np.full((nk, 4), float(p + 1))
        dropped_seq += int((seq.call(u, tau, t, H, STEPS, SUB)[3] & dr.CMD_DROPPED != 0).sum())
        for b, ln in enumerate(f.lines):                     # Fleet.call, opened up between the send and the flight
            assert ln.send(u[b], tau[b], t) == 0, (p, b)
            assert len(ln.fifo) <= 3, (p, b)
            arr = [a for a, _ in ln.fifo]
            assert all(y >= x for x, y in zip(arr, arr[1:]))
            for tk in dr.tick_times(t, H, STEPS, SUB):
                ln.tick(tk)
        t += DT
    assert all(ln.u[0] >= 37.0 for ln in f.lines)            # two periods behind, not stuck
    assert dropped_seq > 0                                   # the sequential rule starves at the same latencies


def test_transport_never_reorders_when_the_latencies_fall():
    ln = rr.Line(rr.RULE_TRANSPORT)
    taus = [3.2 * DT, 2.1 * DT, 1.0 * DT, 0.3 * DT]           # raw arrivals 3.2, 3.1, 3.0, 3.3 periods
    t = 0.0
    for p, ta in enumerate(taus):
        assert ln.send(np.full(4, float(p + 1)), ta, t) == 0
        t += DT
    arr = [a for a, _ in ln.fifo]
    assert arr[0] == arr[1] == arr[2] == 3.2 * DT and arr[3] > arr[2]      # clamped, then free again
    ln.tick(3.2 * DT)
    assert ln.u[0] == 3.0 and len(ln.fifo) == 1              # the three leave in order, the last of them flies


def test_both_rules_agree_up_to_one_period():
    nk = 4
    rng = np.random.default_rng(8)
    a, b = rr.Fleet(nk, np.zeros(nk)), rr.Fleet(nk, np.ones(nk))
    t = 0.0
    for p in range(30):
        tau = rng.choice([0.0, 0.2 * DT, 0.7 * DT, DT], size=nk)
        u = rng.uniform(-0.2, 0.2, (nk, 4))
        ra, rb = a.call(u, tau, t, H, STEPS, SUB), b.call(u, tau, t, H, STEPS, SUB)
        rows = rb[1].copy()
        rows[:, rr.RULE] = 0.0
        np.testing.assert_array_equal(rows, ra[1])
        np.testing.assert_array_equal(ra[0], rb[0])
        t += DT


def test_segments():
    D, ds = 0.1, 16
    u = np.array([0.1, 0.02, -0.03])
    row = np.zeros(rr.INFLIGHT_N)
    row[5:8] = u
    (u0, h, n), = rr.segments(row, D, ds)                     # no switch: today's arithmetic
    assert (h, n) == (D / ds, ds) and np.array_equal(u0, u)
    row[0], row[1], row[8:11] = 1.0, D, [1.0, 2.0, 3.0]       # a switch exactly at the end is none
    assert [(h, n) for _, h, n in rr.segments(row, D, ds)] == [(D / ds, ds)]
    row[1] = 0.0                                              # a switch at 0 skips the first piece
    (u1, h, n), = rr.segments(row, D, ds)
    assert (h, n) == (D / ds, ds) and u1.tolist() == [1.0, 2.0, 3.0]
    rng = np.random.default_rng(2)
    for _ in range(200):
        k = int(rng.integers(0, 5))
        row = np.zeros(rr.INFLIGHT_N)
        row[0] = k
        row[1:1 + k] = np.maximum.accumulate(rng.choice([0.0, 0.013, 0.05, 0.05, 0.0999, 0.1, 0.17], size=k)) if k else []
        row[5:20] = rng.uniform(-1, 1, 15)
        segs = rr.segments(row, D, ds)
        assert 1 <= len(segs) <= 5
        lens = []
        for _, h, n in segs:
            assert 1 <= n <= ds and h > 0.0 and h <= (D / ds) * (1 + 2 ** -50)
            assert n == 1 or float(n - 1) * (D / ds) < n * h          # the smallest n that covers the piece
            lens.append(n * h)
        assert abs(math.fsum(lens) - D) <= len(segs) * math.ulp(D)


def test_inflight_row_model():
    line = rr.Line(rr.RULE_TRANSPORT)
    line.u = np.array([0.1, 0.2, 0.3, 9.0])
    line.send([1.0, 2.0, 3.0, 4.0], 0.07, 1.0)
    line.send([5.0, 6.0, 7.0, 8.0], 0.01, 1.05)               # clamped behind the first
    r = rr.inflight_row(line.as_row(), 1.05)
    assert r[0] == 2 and r[1] == (1.0 + 0.07) - 1.05 and r[2] == r[1] and not r[3:5].any()
    assert r[5:8].tolist() == [0.1, 0.2, 0.3] and r[8:14].tolist() == [1.0, 2.0, 3.0, 5.0, 6.0, 7.0] and not r[14:].any()
    row = line.as_row()
    row[dr.U + 3] = np.nan                                    # the 4th control is ignored
    assert rr.inflight_row(row, 1.05)[0] == 2
    row[dr.U + 1] = np.inf
    bad = rr.inflight_row(row, 1.05)
    assert bad[0] == -1 and not bad[1:].any()


def test_actuation_delay_takes_a_rule_and_reset_writes_the_slot():
    with pytest.raises(ValueError):
        ActuationDelay(3, 0.1, rule="fifo")
    d = ActuationDelay(3, 0.1, rule="transport")
    want = np.zeros((3, nmpc.DELAY_NLINE))
    want[:, nmpc.DELAY_RULE] = 1.0
    np.testing.assert_array_equal(d.line.numpy(), want)
    d.line.fill_(7.0)
    d.reset()
    np.testing.assert_array_equal(d.line.numpy(), want)
    s = ActuationDelay(3, 0.1)
    s.line.fill_(7.0)
    s.reset()
    assert s.rule == "sequential" and not s.line.any()


def test_delay_comp_queue_needs_a_delayed_plant():
    from openkite_amd.fleet import FleetLoop, GpuPlant
    from test_fleet import DT as DTF, N, OracleStepper, initial_states
    x0 = initial_states(0, 3)
    with pytest.raises(ValueError, match="delayed plant"):
        FleetLoop(OracleStepper(3), x0, N, DTF, delay_comp="queue")
    with pytest.raises(ValueError, match="delayed plant"):
        FleetLoop(OracleStepper(3), x0, N, DTF, plant=GpuPlant(None, DTF / 2, 2, 4), delay_comp="queue")
    with pytest.raises(ValueError):
        FleetLoop(OracleStepper(3), x0, N, DTF, delay_comp="fifo")
    lp = FleetLoop(OracleStepper(3), x0, N, DTF, plant=GpuPlant(None, DTF / 2, 2, 4, delay=ActuationDelay(3, 0.1)),
                   delay_comp="queue")
    assert lp.delay_comp == "queue"
    assert FleetLoop(OracleStepper(3), x0, N, DTF).delay_comp == "last"


# ---- GPU -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(kp):
    from oracle import ffi
    rng = np.random.default_rng(31415)
    x13 = ffi.synthetic_states(B, offset=4100)
    u = np.zeros((PERIODS, B, 4))
    u[:, :, 0] = rng.uniform(0.1, 0.15, (PERIODS, B))
    u[:, :, 1:3] = rng.uniform(-0.12, 0.12, (PERIODS, B, 2))
    u[:, :, 3] = rng.uniform(-1.0, 1.0, (PERIODS, B))          # carried by the line, ignored by the plant
    P = ok.perturb_params(kp, B, 0.1, seed=12)
    w8 = np.zeros((B, 8))
    w8[:, 0:3] = rng.uniform(-0.5, 0.5, (B, 3)) / math.sqrt(3.0)
    # 14 kites per latency pair (b % 7, b % 2): every latency meets both rules
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
def g(ctx70, data):
    ctx70.plant_set_params(data["P"])
    ctx70.plant_set_wind(data["w8"][:, 0:3])
    ctx70.use_own_stream()
    return ctx70


def compose(g, x, u_steps, t0):
    st = np.zeros(x.shape[0], dtype=np.int32)
    for j in range(STEPS):
        x, s = g.plant_step(x, u_steps[j], t0 + float(j * SUB) * HS, H, 1, SUB)
        st |= s
    return x, st


def fresh_lines(rules):
    line = np.zeros((len(rules), ok.DELAY_NLINE))
    line[:, nmpc.DELAY_RULE] = rules
    return line


def fly(g, x13, u, tau, rules, send=lambda p: True):
    """PERIODS delayed calls against the model and the composed plant, every
    output compared bitwise each period; returns the per-period outputs."""
    nk = x13.shape[0]
    ref = rr.Fleet(nk, rules)
    x, xr = x13.copy(), x13.copy()
    line = fresh_lines(rules)
    out, t = [], 0.0
    for p in range(PERIODS):
        cmd = u[p] if send(p) else None
        x, line, ua, st = g.plant_step_delayed(x, cmd, tau[p] if cmd is not None else None, line, t, H, STEPS, SUB)
        u_steps, rows, ua_ref, bits = ref.call(cmd, tau[p], t, H, STEPS, SUB)
        xr, nan_bits = compose(g, xr, u_steps, t)
        assert np.array_equal(line, rows, equal_nan=True), f"line, period {p}"
        np.testing.assert_array_equal(ua, ua_ref, err_msg=f"u_applied, period {p}")
        np.testing.assert_array_equal(st, bits | nan_bits, err_msg=f"status, period {p}")
        assert np.array_equal(x, xr, equal_nan=True), f"state, period {p}"
        out.append(dict(x=x.copy(), line=line.copy(), ua=ua.copy(), st=st.copy()))
        t += DT
    return out


@pytest.mark.gpu
def test_mixed_rules_in_one_launch(g, data):
    out = fly(g, data["x13"], data["u"], data["tau_b"], RULES)
    dropped = np.zeros(B, dtype=bool)
    for o in out:
        dropped |= (o["st"] & ok.PLANT_CMD_DROPPED) != 0
        np.testing.assert_array_equal(o["line"][:, nmpc.DELAY_RULE], RULES)       # delay_finish carries the slot
    lat = np.arange(B) % len(TAU_CYCLE)
    # 4.7 periods overflow the depth under both rules; two periods starve the sequential rule only
    assert dropped[(lat == 6) & (RULES == 0)].all() and dropped[(lat == 6) & (RULES == 1)].all()
    assert dropped[(lat == 4) & (RULES == 0)].all() and not dropped[(lat == 4) & (RULES == 1)].any()
    assert not dropped[lat < 4].any()
    # the sequential lines of the mixed launch are an all-sequential launch's
    allseq = fly(g, data["x13"], data["u"], data["tau_b"], np.zeros(B))
    sel = RULES == 0
    for p in range(PERIODS):
        for k in ("x", "line", "ua", "st"):
            np.testing.assert_array_equal(out[p][k][sel], allseq[p][k][sel], err_msg=f"{k}, period {p}")
    # and a NaN in the slot is the sequential rule
    nan_rules = np.where(RULES == 0, np.nan, 1.0)
    got = fly(g, data["x13"], data["u"], data["tau_b"], nan_rules)
    for p in range(PERIODS):
        for k in ("x", "ua", "st"):
            np.testing.assert_array_equal(got[p][k], out[p][k], err_msg=f"{k}, period {p}")


@pytest.mark.gpu
def test_falling_latencies_do_not_reorder_under_either_rule(g, data):
    fall = np.array([3.2, 2.1, 1.0, 0.3, 0.0, 0.0, 0.0, 0.0]) * DT
    tau = fall[:, None] * (1.0 + 0.01 * (np.arange(B) % 5))[None, :]
    out = fly(g, data["x13"], data["u"], tau, RULES)
    for o in out:
        n = o["line"][:, nmpc.DELAY_COUNT].astype(int)
        for b in range(B):
            assert np.all(np.diff(o["line"][b, nmpc.DELAY_T_ARR:nmpc.DELAY_T_ARR + n[b]]) >= 0)
    np.testing.assert_array_equal(out[-1]["ua"], data["u"][-1])                   # everything got through, in order


@pytest.mark.gpu
def test_periods_without_a_command(g, data):
    out = fly(g, data["x13"], data["u"], data["tau_b"], RULES, send=lambda p: p % 3 != 1)
    assert any(o["line"][:, nmpc.DELAY_COUNT].any() for o in out)


@pytest.mark.gpu
def test_bad_tau_and_non_finite_kites(g, data):
    tau = np.array(data["tau_b"])
    tau[:, 4], tau[:, 5] = np.nan, -0.01                      # one of each rule
    tau[2:, 66], tau[2:, 67] = np.inf, np.nan                 # after two accepted commands
    x = data["x13"].copy()
    x[10, 0], x[69, 11] = np.nan, np.inf                      # non-finite on entry
    x[3, 0] = 1e160                                           # overflows in the first substep
    out = fly(g, x, data["u"], tau, RULES)
    clean = fly(g, data["x13"], data["u"], tau, RULES)
    for p in range(PERIODS):
        assert out[p]["st"][4] & ok.PLANT_BAD_TAU and out[p]["st"][5] & ok.PLANT_BAD_TAU
        assert bool(out[p]["st"][66] & ok.PLANT_BAD_TAU) == (p >= 2) == bool(out[p]["st"][67] & ok.PLANT_BAD_TAU)
        for b in (3, 10, 69):
            assert out[p]["st"][b] & ok.PLANT_NAN and np.array_equal(out[p]["x"][b], x[b], equal_nan=True)
        np.testing.assert_array_equal(out[p]["line"], clean[p]["line"])            # the queue does not look at the state
        np.testing.assert_array_equal(out[p]["ua"], clean[p]["ua"])


@pytest.mark.gpu
def test_device_and_host_entry_points_agree(g, data):
    want = fly(g, data["x13"], data["u"], data["tau_b"], RULES, send=lambda p: p != 3)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        x = torch.from_numpy(data["x13"].copy()).cuda()
        line = torch.from_numpy(fresh_lines(RULES)).cuda()
        ua = torch.full((B, 4), 7.0, dtype=torch.float64, device="cuda")
        st = torch.full((B,), 77, dtype=torch.int32, device="cuda")
        t = 0.0
        for p in range(PERIODS):
            u = torch.from_numpy(data["u"][p].copy()).cuda()
            tau = torch.from_numpy(data["tau_b"][p].copy()).cuda()
            g.plant_step_delayed_device(x.data_ptr(), u.data_ptr() if p != 3 else 0, tau.data_ptr() if p != 3 else 0,
                                        line.data_ptr(), t, H, STEPS, SUB, ua.data_ptr(), st.data_ptr())
            torch.cuda.synchronize()
            for got, k in ((x, "x"), (line, "line"), (ua, "ua"), (st, "st")):
                np.testing.assert_array_equal(got.cpu().numpy(), want[p][k], err_msg=f"{k}, period {p}")
            t += DT
    finally:
        g.use_own_stream()
