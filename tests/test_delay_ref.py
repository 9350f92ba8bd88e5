"""The command-line reference model (tests/delay_ref.py) checked against the
semantics it restates, and the delayed plant's public surface (CPU): both C
symbols exported, API version unchanged, the Python wrappers refuse wrong
shapes before they reach the library."""
import types

import numpy as np
import pytest

import openkite_amd as ok
from openkite_amd import nmpc

import delay_ref as dr

H, STEPS, SUB = 0.02, 3, 2
DT = STEPS * H


def cmds(B, periods, seed=5):
    return np.random.default_rng(seed).uniform(-0.2, 0.2, (periods, B, 4))


def test_layout_matches_the_python_constants():
    assert (dr.DEPTH, dr.NLINE) == (nmpc.DELAY_DEPTH, nmpc.DELAY_NLINE) == (ok.DELAY_DEPTH, ok.DELAY_NLINE) == (4, 32)
    assert (dr.COUNT, dr.T_PREV, dr.HAS_PREV, dr.U_FORCE, dr.T_ARR, dr.U) == (
        nmpc.DELAY_COUNT, nmpc.DELAY_T_PREV, nmpc.DELAY_HAS_PREV, nmpc.DELAY_U_FORCE, nmpc.DELAY_T_ARR, nmpc.DELAY_U)
    assert (dr.CMD_DROPPED, dr.BAD_TAU) == (ok.PLANT_CMD_DROPPED, ok.PLANT_BAD_TAU) == (2, 4)
    assert not dr.Line().as_row().any()                       # a fresh line is the all-zero row


def test_tick_times_are_the_hosts():
    hs = H / SUB
    assert dr.tick_times(0.18, H, STEPS, SUB) == [0.18 + 0.0 * hs, 0.18 + 2.0 * hs, 0.18 + 4.0 * hs]


def test_zero_latency_is_the_identity():
    B, P = 3, 6
    u = cmds(B, P)
    f, t = dr.Fleet(B), 0.0
    for p in range(P):
        us, rows, ua, bits = f.call(u[p], np.zeros(B), t, H, STEPS, SUB)
        for j in range(STEPS):
            np.testing.assert_array_equal(us[j], u[p])        # t_arr == t_0: in force from the first tick
        np.testing.assert_array_equal(ua, u[p])
        assert not bits.any() and not rows[:, dr.COUNT].any()
        np.testing.assert_array_equal(rows[:, dr.T_PREV], t)
        t += DT


def test_arrivals_never_reorder_under_decreasing_tau():
    f = dr.Fleet(1)
    taus = [2.5 * DT, 1.2 * DT, 0.1 * DT, 0.0]                # raw arrivals t0 + tau would come out reversed
    arr, t = [], 0.0
    for p, ta in enumerate(taus):
        u = np.full((1, 4), float(p + 1))
        _, rows, _, bits = f.call(u, np.array([ta]), t, H, STEPS, SUB)
        arr.append(rows[0, dr.T_PREV])
        assert not bits.any()
        t += DT
    assert all(b >= a for a, b in zip(arr, arr[1:])) and arr[0] == 2.5 * DT
    assert arr[1] == arr[0] + 1.2 * DT                         # max(t_send, t_arr_prev) + tau
    # they leave in the order they were sent
    seen = []
    for _ in range(12):
        us, _, _, _ = f.call(None, None, t, H, STEPS, SUB)
        seen += [us[j, 0, 0] for j in range(STEPS)]
        t += DT
    changes = [v for i, v in enumerate(seen) if i == 0 or v != seen[i - 1]]
    assert changes == sorted(changes) and changes[-1] == 4.0


def test_a_full_line_drops_its_oldest_command():
    f = dr.Fleet(1)
    t = 0.0
    for p in range(6):
        _, rows, ua, bits = f.call(np.full((1, 4), float(p + 1)), np.array([100.0]), t, H, STEPS, SUB)
        assert bits[0] == (dr.CMD_DROPPED if p >= dr.DEPTH else 0)
        assert rows[0, dr.COUNT] == min(p + 1, dr.DEPTH)
        assert not ua.any()                                   # nothing has arrived
        t += DT
    np.testing.assert_array_equal(rows[0, dr.U:dr.U + 16:4], [3.0, 4.0, 5.0, 6.0])      # 1 and 2 are gone
    assert np.all(np.diff(rows[0, dr.T_ARR:dr.T_ARR + 4]) == 100.0)


@pytest.mark.parametrize("bad", [np.nan, -1e-3, np.inf, -np.inf])
def test_a_bad_tau_drops_the_command(bad):
    f = dr.Fleet(2)
    u = cmds(2, 1)[0]
    us, rows, ua, bits = f.call(u, np.array([bad, 0.0]), 0.0, H, STEPS, SUB)
    assert bits.tolist() == [dr.BAD_TAU, 0]
    assert not rows[0].any() and not ua[0].any()              # the line is as it was: fresh
    np.testing.assert_array_equal(ua[1], u[1])


def test_the_delayed_plant_is_exported_and_the_wrappers_refuse_wrong_shapes():
    L = ok.lib()
    assert L.kite_nmpc_api_version() == 7
    for name in ("kite_nmpc_plant_step_delayed", "kite_nmpc_plant_step_delayed_device"):
        assert hasattr(L, name) and name in nmpc._SIGNATURES
    B = 3
    fake = types.SimpleNamespace(batch=B, _h=None)            # the shape checks come before the library call
    good = dict(x13=np.zeros((B, 13)), u4_cmd=np.zeros((B, 4)), tau=np.zeros(B), line=np.zeros((B, ok.DELAY_NLINE)))
    for key, wrong in (("x13", np.zeros((B, 15))), ("x13", np.zeros((B + 1, 13))), ("u4_cmd", np.zeros((B, 3))),
                       ("tau", np.zeros((B, 1))), ("tau", np.zeros(B + 1)), ("tau", None),
                       ("line", np.zeros((B, 31))), ("line", np.zeros(B * 32))):
        a = dict(good)
        a[key] = wrong
        with pytest.raises(ValueError):
            ok.BatchNMPC.plant_step_delayed(fake, a["x13"], a["u4_cmd"], a["tau"], a["line"], 0.0, H, STEPS, SUB)


def test_actuation_delay_draws_in_range_and_resets():
    from openkite_amd.fleet import ActuationDelay
    d = ActuationDelay(50, 0.02, 0.005, seed=3)
    a = d.draw().clone()
    assert a.shape == (50,) and bool((a >= 0.015).all()) and bool((a <= 0.025).all()) and a.std() > 0
    b = d.draw().clone()
    assert not np.array_equal(a.numpy(), b.numpy())
    d.line.fill_(1.0)
    d.u_applied.fill_(1.0)
    d.reset()
    assert not d.line.any() and not d.u_applied.any()
    np.testing.assert_array_equal(d.draw().numpy(), a.numpy())            # the generator is back at its seed
    lo = ActuationDelay(4, 0.002, 0.005)
    assert lo.lo == 0.0 and lo.hi == 0.007                                # max(mean - deviation, 0)
    const = ActuationDelay(4, 0.1)
    np.testing.assert_array_equal(const.draw().numpy(), 0.1)
    with pytest.raises(ValueError):
        ActuationDelay(4, -0.1)


def test_a_recorder_needs_a_control_that_is_constant_over_the_period():
    """(l) of the GPU cases, which needs none: the rule is checked at construction."""
    import torch
    from openkite_amd.fleet import ActuationDelay, FleetLoop, FlightRecorder, GpuPlant
    from test_fleet import DT as DTF, N, OracleStepper, initial_states
    nk = 3
    x0 = initial_states(0, nk)

    def loop(mean, dev):
        plant = GpuPlant(None, DTF / 2, 2, 4, delay=ActuationDelay(nk, mean, dev))
        return FleetLoop(OracleStepper(nk), x0, N, DTF, plant=plant, recorder=FlightRecorder(nk, 4))

    with pytest.raises(ValueError, match="deviation"):
        loop(2 * DTF, 0.005)
    with pytest.raises(ValueError, match="whole number"):
        loop(1.5 * DTF, 0.0)
    for k in (0, 1, 2):
        loop(k * DTF, 0.0)
    # without a recorder any delay is accepted, and one of another batch is not
    FleetLoop(OracleStepper(nk), x0, N, DTF, plant=GpuPlant(None, DTF / 2, 2, 4, delay=ActuationDelay(nk, 0.02, 0.005)))
    with pytest.raises(ValueError):
        FleetLoop(OracleStepper(nk), x0, N, DTF, plant=GpuPlant(None, DTF / 2, 2, 4, delay=ActuationDelay(nk + 1, 0.02)))
    assert torch.is_tensor(x0)
