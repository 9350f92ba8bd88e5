"""Pure-Python float64 models of the command line's two arrival rules, of the
in-flight schedule row (k_inflight) and of the substep rule of the queue-aware
delay compensation (prologue_kite): test infrastructure, next to delay_ref.py.

  rule     slot RULE (3) of the line's row: exactly 1.0 is the transport rule,
           t_arr = max(t_send + tau, t_arr_prev) with t_arr_prev counted only
           once a command has been accepted; any other value is delay_ref's
           sequential rule, t_arr = max(t_send, t_arr_prev) + tau.
  schedule ``inflight_row(row, t0)``: [n | s_1..s_4 | control in force (3) |
           pending commands (4 x 3) | zeros]; n the pending count as the send
           reads it, s_i = max(t_arr_i - t0, 0) then a running maximum; a
           non-finite control in force, arrival time or (T, dE, dR) of a
           pending command: n = -1 and the rest zero.
  pieces   ``segments(sched_row, D, delay_steps)``: the window [0, D] cut at
           the switches inside it, [(u3, h, n)] with n substeps of h each.
"""
import math

import numpy as np

import delay_ref as dr

RULE, RULE_SEQUENTIAL, RULE_TRANSPORT = 3, 0.0, 1.0
INFLIGHT_N = 24


class Line(dr.Line):
    """delay_ref.Line with the rule slot: ``rule`` is the slot's value."""

    def __init__(self, rule=RULE_SEQUENTIAL):
        super().__init__()
        self.rule = float(rule)

    def send(self, u_cmd, tau, t_send):
        if self.rule != RULE_TRANSPORT:             # NaN and every other value: the sequential rule
            return super().send(u_cmd, tau, t_send)
        tau = float(tau)
        if not (tau >= 0.0) or not math.isfinite(tau):
            return dr.BAD_TAU
        t_arr = t_send + tau
        if self.t_prev is not None:
            t_arr = max(t_arr, self.t_prev)         # the channel never reorders
        bits = 0
        if len(self.fifo) == dr.DEPTH:
            self.fifo.pop(0)
            bits = dr.CMD_DROPPED
        self.fifo.append((t_arr, np.array(u_cmd, dtype=np.float64)))
        self.t_prev = t_arr
        return bits

    def as_row(self):
        r = super().as_row()
        r[RULE] = self.rule
        return r


class Fleet(dr.Fleet):
    """B lines, ``rules`` (B,) their rule slots."""

    def __init__(self, B, rules=None):
        rules = np.zeros(B) if rules is None else np.asarray(rules, dtype=np.float64)
        self.lines = [Line(rules[b]) for b in range(B)]


def count(row):
    """The pending count as delay_send reads it: 0 .. DEPTH, NaN: 0."""
    c = row[dr.COUNT]
    return (dr.DEPTH if c >= float(dr.DEPTH) else int(c)) if c >= 1.0 else 0


def inflight_row(row, t0):
    """The schedule row of the line ``row`` (32 doubles) seen at time t0."""
    n = count(row)
    r = np.zeros(INFLIGHT_N)
    r[5:8] = row[dr.U_FORCE:dr.U_FORCE + 3]
    ok = bool(np.all(np.isfinite(r[5:8])))
    run = 0.0
    for s in range(n):
        ta = row[dr.T_ARR + s]
        cmd = row[dr.U + 4 * s:dr.U + 4 * s + 3]
        if not math.isfinite(ta) or not np.all(np.isfinite(cmd)):
            ok = False
            continue
        run = max(run, max(ta - t0, 0.0))
        r[1 + s] = run
        r[8 + 3 * s:11 + 3 * s] = cmd
    if not ok:
        r[:] = 0.0
        r[0] = -1.0
        return r
    r[0] = float(n)
    return r


def inflight_rows(rows, t0):
    return np.stack([inflight_row(r, t0) for r in rows])


def substeps(L, h_max, delay_steps):
    n = 1
    while n < delay_steps and float(n) * h_max < L:
        n += 1
    return n


def segments(sched_row, D, delay_steps):
    """[(u3, h, n)]: the pieces of [0, D] under a valid schedule row, in order.
    A switch at or beyond D is none; a zero-length piece is skipped."""
    nsw = int(sched_row[0])
    assert nsw >= 0, "an invalid row has no pieces: the step predicts under the previous u(t0)"
    h_max = D / delay_steps
    u = np.array(sched_row[5:8])
    out, a = [], 0.0
    for seg in range(nsw + 1):
        e = min(sched_row[1 + seg], D) if seg < nsw else D
        L = e - a
        if L > 0.0:
            n = substeps(L, h_max, delay_steps)
            out.append((u.copy(), L / n, n))
            a = e
        if seg < nsw:
            u = np.array(sched_row[8 + 3 * seg:11 + 3 * seg])
    return out
