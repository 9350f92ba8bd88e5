"""The sensitivity and condensing kernels after their loop-shape changes
(k_rk4_sens1 / k_rk4_sens2 with the RK4 stages peeled at both ends,
k_condense20's propagation): nothing they produce may move.

* a small batch (B = 5: no multiple of 4, below the k_rk4_sens1 switch), one
  cold and two warm steps: [A | B] and the defects of every interval and the
  condensed QP against the oracle, at test_gpu_parity.py's bars for those
  quantities (x+ 1e-12, S 1e-10, QP 1e-11);
* B = 129 takes k_rk4_sens2 where B = 5 takes k_rk4_sens1: its first 5 kites
  equal the B = 5 run bitwise, plans, QPs and sensitivities;
* condensing seeds: a kite linearised around a plan with controls exactly at
  their bounds and a kite with a state exactly 0.0 give the H, h and C that
  tests/golden/condense_seeds_golden.npz records from the commit before the
  change (tests/golden/gen_condense_seeds_golden.py), bit for bit.
"""
import os

import numpy as np
import pytest

import openkite_amd as ok
from oracle import ffi
from test_gpu_parity import M, N, condensed_cfgv, gpu_to_oracle_perm, rel, x0_batch

pytestmark = pytest.mark.gpu

B_SMALL, B_LARGE, STEPS = 5, 129, 3
QP_TOL = 1e-11      # condensed QP (H, h, C) against the oracle, test_gpu_parity.py
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "condense_seeds_golden.npz")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def closed_loop(B):
    """STEPS steps of B kites (cold, then warm on the plan's own prediction).
    Per step: the measured state, the plan the step started from, the plan it
    returned, the QP of the first B_SMALL kites, and the sensitivities of the
    returned plan's intervals for those kites through the context's own
    sensitivity kernel (B_SMALL * N items for B = 5: k_rk4_sens1; padded with
    copies of the last item to B * N for B = 129: k_rk4_sens2)."""
    cfg = ok.default_config()
    g = ok.BatchNMPC(ok.load_properties(), cfg, B)
    x = x0_batch(B)
    out = []
    try:
        for s in range(STEPS):
            before = g.get_solution()
            r = g.step(x)
            qp = [g.get_qp(b) for b in range(B_SMALL)]
            xs = r["traj"][:B_SMALL, :N, :].reshape(-1, 15)
            us = r["ctrl"][:B_SMALL].reshape(-1, 4)
            pad = B * N - xs.shape[0]
            xo, A, Bm = g.rk4_sens(np.vstack([xs, np.repeat(xs[-1:], pad, 0)]),
                                   np.vstack([us, np.repeat(us[-1:], pad, 0)]), cfg.dt, M)
            n = xs.shape[0]
            out.append(dict(x=x[:B_SMALL].copy(), before=[a[:B_SMALL].copy() for a in before], u0=r["u0"][:B_SMALL].copy(),
                            traj=r["traj"][:B_SMALL].copy(), ctrl=r["ctrl"][:B_SMALL].copy(), qp=qp,
                            sx=xs, su=us, xo=xo[:n].copy(), A=A[:n].copy(), Bm=Bm[:n].copy()))
            x = r["traj"][:, 1, :].copy()
    finally:
        g.close()
    return out, float(cfg.dt)


@pytest.fixture(scope="module")
def small():
    return closed_loop(B_SMALL)


@pytest.fixture(scope="module")
def large():
    return closed_loop(B_LARGE)


def test_small_batch_sens_and_qp_vs_oracle(small, kp):
    steps, dt = small
    cfgv = condensed_cfgv()
    perm = gpu_to_oracle_perm(N)
    for s, st in enumerate(steps):
        # [A | B] and the defect's x+ of every interval of the returned plan
        for i in range(st["sx"].shape[0]):
            xr, Ar, Br = ffi.rk4_sens(kp, st["sx"][i], st["su"][i], dt / M, M)
            ex, eA, eB = rel(st["xo"][i], xr), rel(st["A"][i], Ar), rel(st["Bm"][i], Br)
            assert ex < 1e-12 and eA < 1e-10 and eB < 1e-10, (s, i, ex, eA, eB)
        # the condensed QP, the oracle linearised where the GPU step was
        # (its prologue on the plan the GPU step started from)
        for b in range(B_SMALL):
            Xb, Ub = st["before"][0][b], st["before"][1][b]
            _, X, U, _ = ffi.prologue(kp, cfgv, N, M, st["x"][b], Xb, Ub, warm=int(s > 0))
            q = ffi.build_qp(kp, cfgv, N, M, X, U)
            gq = st["qp"][b]
            Hg = np.zeros_like(q["H"]); Hg[np.ix_(perm, perm)] = gq["H"]
            hg = np.zeros_like(q["h"]); hg[perm] = gq["h"]
            Cg = np.zeros((N, 4 * N + 2)); Cg[:, perm] = gq["C"]
            eH = np.abs(Hg - q["H"]).max() / np.abs(q["H"]).max()
            eh = np.abs(hg - q["h"]).max() / max(1.0, np.abs(q["h"]).max())
            eC = np.abs(Cg - q["C"]).max() / max(1.0, np.abs(q["C"]).max())
            print(f"step {s} kite {b}: H {eH:.2e} h {eh:.2e} C {eC:.2e}")
            assert eH < QP_TOL and eh < QP_TOL and eC < QP_TOL, (s, b, eH, eh, eC)


def test_first_kites_bitwise_across_the_sens_switch(small, large):
    for s, (a, c) in enumerate(zip(small[0], large[0])):
        for k in ("u0", "traj", "ctrl", "xo", "A", "Bm"):
            assert np.array_equal(bits(a[k]), bits(c[k])), (s, k)
        for b in range(B_SMALL):
            for k in ("H", "h", "C", "cl", "cu"):
                assert np.array_equal(bits(a["qp"][b][k]), bits(c["qp"][b][k])), (s, b, k)


UP = (6, 1)     # (interval, control) planted at its upper bound, kite 0
LO = (9, 2)     # (interval, control) planted at its lower bound, kite 0


def seed_inputs():
    x0 = x0_batch(2, offset=7000)
    x0[1, 4] = 0.0
    return x0


def run_seed_case(x0, x1=None, plan=None):
    """Cold step on x0, plant the plan, warm step on x1; the inputs and both
    kites' QPs after each step.  Without x1 and a plan (recording the golden
    file) they are made from the cold step: the returned plan with kite 0's
    controls UP and LO put exactly on their bounds, the predicted next state
    with kite 1's wy put back to exactly 0.0."""
    cfg = ok.default_config()
    g = ok.BatchNMPC(ok.load_properties(), cfg, 2)
    try:
        r = g.step(x0)
        cold = [g.get_qp(b) for b in range(2)]
        if plan is None:
            traj, ctrl = g.get_solution()
            lbu, ubu = np.array(cfg.lbu), np.array(cfg.ubu)
            assert np.isfinite(ubu[UP[1]]) and np.isfinite(lbu[LO[1]])
            ctrl[0, UP[0], UP[1]] = ubu[UP[1]]
            ctrl[0, LO[0], LO[1]] = lbu[LO[1]]
            x1 = r["traj"][:, 1, :].copy()
            x1[1, 4] = 0.0
        else:
            traj, ctrl = plan
        g.set_solution(traj, ctrl)
        g.step(x1)
        warm = [g.get_qp(b) for b in range(2)]
    finally:
        g.close()
    out = dict(x0=x0, x1=x1, traj=traj, ctrl=ctrl)
    for tag, qs in (("cold", cold), ("warm", warm)):
        for k in ("H", "h", "C"):
            out[f"{tag}_{k}"] = np.array([q[k] for q in qs])
    return out


def test_condensing_seeds_bitwise_vs_recorded():
    gold = np.load(GOLDEN)
    cfg = ok.default_config()
    # the recorded inputs are the cases the file is for
    assert gold["ctrl"][0, UP[0], UP[1]] == cfg.ubu[UP[1]] and gold["ctrl"][0, LO[0], LO[1]] == cfg.lbu[LO[1]]
    assert gold["x0"][1, 4] == 0.0 and gold["x1"][1, 4] == 0.0
    assert np.array_equal(bits(gold["x0"]), bits(seed_inputs()))
    got = run_seed_case(gold["x0"], gold["x1"], (gold["traj"], gold["ctrl"]))
    for tag in ("cold", "warm"):
        for k in ("H", "h", "C"):
            a, c = got[f"{tag}_{k}"], gold[f"{tag}_{k}"]
            assert np.all(np.isfinite(c)) and np.abs(c).max() > 0.0, (tag, k)
            ne = bits(a) != bits(c)
            assert not ne.any(), (tag, k, int(ne.sum()), float(np.abs(a - c).max()))
