"""Pure-Python float64 model of the per-kite command line of the delayed plant
(kite_nmpc_plant_step_delayed, k_plant_delay): test infrastructure.

A line is the control in force plus a FIFO of at most DEPTH pending commands
with their arrival times.  One call is one control period of ``steps`` plant
steps of ``h``:

  send   a command sent at t0 with latency tau arrives at max(t0, t_arr_prev) +
         tau, t_arr_prev the arrival of the last accepted command (t0 if there
         is none).  tau negative or non-finite: dropped, BAD_TAU.  A send to a
         full line drops the oldest pending command, CMD_DROPPED.
  fly    before plant step j every pending command with t_arr <= t_j leaves the
         FIFO in order and the last of them becomes the control in force;
         t_j = t0 + float(j * substeps) * hs with hs = h / substeps, the product
         rounded, then the sum: the host's and plant_time's arithmetic.
  report u_applied is the control in force during the last plant step.

``Line.as_row`` is the 32-double row of the C ABI (slots KITE_DELAY_*).
"""
import math

import numpy as np

DEPTH, NLINE = 4, 32
COUNT, T_PREV, HAS_PREV, U_FORCE, T_ARR, U = 0, 1, 2, 4, 8, 12
CMD_DROPPED, BAD_TAU = 2, 4


def tick_times(t0, h, steps, substeps):
    hs = h / substeps
    return [t0 + float(j * substeps) * hs for j in range(steps)]


class Line:
    """One kite's line.  A fresh one is the all-zero row."""

    def __init__(self):
        self.u = np.zeros(4)            # the control in force
        self.fifo = []                  # [(t_arr, u (4,))], oldest first
        self.t_prev = None              # arrival of the last accepted command

    def send(self, u_cmd, tau, t_send):
        """Returns the status bits of the send."""
        tau = float(tau)
        if not (tau >= 0.0) or not math.isfinite(tau):
            return BAD_TAU
        prev = t_send if self.t_prev is None else self.t_prev
        t_arr = max(t_send, prev) + tau
        bits = 0
        if len(self.fifo) == DEPTH:
            self.fifo.pop(0)
            bits = CMD_DROPPED
        self.fifo.append((t_arr, np.array(u_cmd, dtype=np.float64)))
        self.t_prev = t_arr
        return bits

    def tick(self, t):
        while self.fifo and self.fifo[0][0] <= t:
            self.u = self.fifo.pop(0)[1]

    def as_row(self):
        r = np.zeros(NLINE)
        r[COUNT] = len(self.fifo)
        if self.t_prev is not None:
            r[T_PREV], r[HAS_PREV] = self.t_prev, 1.0
        r[U_FORCE:U_FORCE + 4] = self.u
        for s, (t_arr, u) in enumerate(self.fifo):
            r[T_ARR + s] = t_arr
            r[U + 4 * s:U + 4 * s + 4] = u
        return r


class Fleet:
    """B lines advanced call by call."""

    def __init__(self, B):
        self.lines = [Line() for _ in range(B)]

    def call(self, u_cmd, tau, t0, h, steps, substeps):
        """One control period.  u_cmd (B, 4) or None (nothing sent), tau (B,).
        Returns (u_steps (steps, B, 4): the control in force at every plant
        step, rows (B, 32): the lines after the call, u_applied (B, 4), bits
        (B,) int32: CMD_DROPPED / BAD_TAU)."""
        B = len(self.lines)
        bits = np.zeros(B, dtype=np.int32)
        u_steps = np.zeros((steps, B, 4))
        ticks = tick_times(t0, h, steps, substeps)
        for b, ln in enumerate(self.lines):
            if u_cmd is not None:
                bits[b] = ln.send(u_cmd[b], tau[b], t0)
            for j, t in enumerate(ticks):
                ln.tick(t)
                u_steps[j, b] = ln.u
        rows = np.stack([ln.as_row() for ln in self.lines])
        return u_steps, rows, u_steps[-1].copy(), bits


def run(calls, B):
    """calls: a sequence of dicts (u_cmd, tau, t0, h, steps, substeps); returns
    the list of ``Fleet.call`` results."""
    f = Fleet(B)
    return [f.call(c.get("u_cmd"), c.get("tau"), c["t0"], c["h"], c["steps"], c["substeps"]) for c in calls]
