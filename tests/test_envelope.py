"""The GPU path across the flight envelope and across batch positions.

Every other parity test draws its kites from the cloud around ffi.BASE_STATE.
Here (states: tests/envelope_states.py, 50-digit fixture:
tests/golden/kite_envelope_golden.json):

  A  kite_rhs and its scalar types off the base state: the oracle (CPU) and
     k_dynamics / k_jacobian / k_rk4_sens1 / k_rk4_sens2 (fp64 and fp32
     tangents) against the fixture, regime by regime
  B  RTI parity around the orbit: condensed QP data, closed-loop steps at
     N = 20 and N = 40, the theta wrap of the prologue (status bit 16), and a
     batch in which every kite restarts cold at once
  C  batch-position invariance, bitwise: natural order, a permutation, an
     interior shard and the tail kite alone, with and without wind
  D  k_ekf at counts that leave its last block partial and at envelope states
"""
import functools
import json
import os

import numpy as np
import pytest

import openkite_amd as ok
from oracle import ffi
from tests.envelope_states import orbit_batch, regime, wrapped

M, K = 2, 16
RHS_TOL, JAC_TOL, RK4_TOL, SENS_TOL = 1e-13, 1e-12, 1e-12, 1e-10      # tests/test_oracle.py

# Per-regime bars, for the oracle and the GPU alike.  A bar leaves the
# project's default only where the ORACLE (plain IEEE double, no fast_rcp)
# misses the default against the 50-digit fixture, which makes that regime
# conditioning-limited; the bar is then 4 x the oracle's measured error (a
# different operation order and <= 1 ulp per fast_rcp).  Never set from a GPU
# result.  The oracle misses no default bar in any regime, so every entry is
# the default; the comment holds the oracle's worst error of the regime
# (f, J by AD and complex step, x+, S) and the largest S_err_prec24.
_DEFAULT = dict(f=RHS_TOL, J=JAC_TOL, xnext=RK4_TOL, S=SENS_TOL)
BARS = {
    "orbit":    dict(_DEFAULT),   # f 8.3e-17  J 1.2e-16  x+ 1.7e-16  S 2.2e-16  prec24 3.5e-7
    "attitude": dict(_DEFAULT),   # f 2.1e-16  J 1.8e-16  x+ 1.0e-16  S 1.1e-15  prec24 3.8e-7
    "airspeed": dict(_DEFAULT),   # f 2.0e-16  J 2.3e-16  x+ 6.9e-16  S 9.0e-16  prec24 1.6e-6
    "aoa":      dict(_DEFAULT),   # f 3.2e-16  J 2.9e-16  x+ 2.3e-16  S 3.1e-16  prec24 2.7e-7
    "sideslip": dict(_DEFAULT),   # f 1.3e-15  J 2.7e-16  x+ 1.4e-16  S 4.8e-16  prec24 2.8e-7
    "tether":   dict(_DEFAULT),   # f 2.4e-16  J 2.4e-16  x+ 3.6e-16  S 3.5e-16  prec24 3.4e-7
    "qnorm":    dict(_DEFAULT),   # f 4.7e-17  J 2.1e-16  x+ 1.8e-16  S 2.2e-16  prec24 1.8e-7
    "controls": dict(_DEFAULT),   # f 1.6e-16  J 1.2e-16  x+ 1.8e-16  S 1.1e-16  prec24 3.8e-7
}
FP32_FLOOR = 1e-4       # test_rk4_sens_hot_kernel_ragged_batch's fp32 bar; every 8 x S_err_prec24 is below it


def bar(source, what):
    return BARS[regime(source)][what]


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.fixture(scope="module")
def env():
    with open(os.path.join(os.path.dirname(__file__), "golden", "kite_envelope_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ctx1():
    c = ok.BatchNMPC(ok.load_properties(), ok.default_config(), 1)
    yield c
    c.close()


# ---- A. envelope goldens ------------------------------------------------------

def test_fixture_covers_every_regime(env):
    regs = [regime(c["source"]) for c in env["rhs"]]
    want = dict(orbit=8, attitude=4, airspeed=3, aoa=4, sideslip=4, tether=8, qnorm=2, controls=8)
    assert {r: regs.count(r) for r in want} == want and len(regs) == sum(want.values())
    rk = [regime(c["source"]) for c in env["rk4"]]
    assert set(rk) == set(want) and rk.count("orbit") == 3
    assert all(c["tf"] == 0.05 and c["M"] == 2 and c["S_err_prec24"] > 0 for c in env["rk4"])


def test_oracle_rhs_vs_envelope_golden(kp, env):
    bad = []
    for c in env["rhs"]:
        e = rel(ffi.rhs(kp, c["x"], c["u"]), c["f"])
        print(f"f {e:.2e} {c['source']}")
        if not e < bar(c["source"], "f"):
            bad.append((c["source"], e))
    assert not bad, bad


@pytest.mark.parametrize("method", ["ad", "cs"])
def test_oracle_jacobian_vs_envelope_golden(kp, env, method):
    bad = []
    for c in env["rhs"]:
        e = rel(ffi.rhs_jac(kp, c["x"], c["u"], method), c["J"])
        print(f"J[{method}] {e:.2e} {c['source']}")
        if not e < bar(c["source"], "J"):
            bad.append((c["source"], e))
    assert not bad, bad


def test_oracle_rk4_sens_vs_envelope_golden(kp, env):
    bad = []
    for c in env["rk4"]:
        xo, A, B = ffi.rk4_sens(kp, c["x"], c["u"], c["tf"] / c["M"], c["M"])
        e = (rel(xo, c["xnext"]), rel(A, c["A"]), rel(B, c["B"]))
        print("x+ %.2e A %.2e B %.2e prec24 %.2e %s" % (*e, c["S_err_prec24"], c["source"]))
        if not (e[0] < bar(c["source"], "xnext") and max(e[1:]) < bar(c["source"], "S")):
            bad.append((c["source"], e))
    assert not bad, bad


@pytest.mark.gpu
def test_gpu_dynamics_vs_envelope_golden(ctx1, env):
    cs = env["rhs"]
    X = np.array([c["x"] + [0.3, -0.2] for c in cs]); U = np.array([c["u"] + [0.5] for c in cs])
    F = ctx1.dynamics(X, U)
    bad = []
    for i, c in enumerate(cs):
        e = rel(F[i, :13], c["f"])
        print(f"f {e:.2e} {c['source']}")
        if not (e < bar(c["source"], "f") and F[i, 13] == -0.2 and F[i, 14] == 0.5):
            bad.append((c["source"], e))
    assert not bad, bad


@pytest.mark.gpu
def test_gpu_jacobian_vs_envelope_golden(ctx1, env):
    cs = env["rhs"]
    Jx, Ju = ctx1.jacobian(np.array([c["x"] for c in cs]), np.array([c["u"] for c in cs]))
    bad = []
    for i, c in enumerate(cs):
        J = np.array(c["J"])
        e = max(rel(Jx[i], J[:, :13]), rel(Ju[i], J[:, 13:]))
        print(f"J {e:.2e} {c['source']}")
        if not e < bar(c["source"], "J"):
            bad.append((c["source"], e))
    assert not bad, bad


def _rk4_inputs(env, count=None):
    cs = env["rk4"]
    X = np.array([c["x"] for c in cs]); U = np.array([c["u"] for c in cs])
    if count is not None:                      # padded by repeating the cases
        idx = np.arange(count) % len(cs)
        X, U = X[idx], U[idx]
    return cs, X, U


@pytest.mark.gpu
def test_gpu_rk4_sens_vs_envelope_golden(ctx1, env):
    """The cases alone (k_rk4_sens1, <= 128 items) and padded to 129 items
    (k_rk4_sens2): both at the fixture's bars, and bitwise equal to each other."""
    cs, X, U = _rk4_inputs(env)
    n = len(cs)
    r1 = ctx1.rk4_sens(X, U, cs[0]["tf"], cs[0]["M"])
    _, X2, U2 = _rk4_inputs(env, 129)
    r2 = ctx1.rk4_sens(X2, U2, cs[0]["tf"], cs[0]["M"])
    bad = []
    for name, (xo, A, B) in (("sens1", r1), ("sens2", r2)):
        for i in range(len(xo)):
            c = cs[i % n]
            e = (rel(xo[i], c["xnext"]), rel(A[i], c["A"]), rel(B[i], c["B"]))
            if i < n:
                print("%s x+ %.2e A %.2e B %.2e %s" % (name, *e, c["source"]))
            if not (e[0] < bar(c["source"], "xnext") and max(e[1:]) < bar(c["source"], "S")):
                bad.append((name, i, c["source"], e))
    assert not bad, bad
    for a, b in zip(r1, r2):
        np.testing.assert_array_equal(a, b[:n])
        np.testing.assert_array_equal(b[:129 - 129 % n], np.tile(b[:n], (129 // n,) + (1,) * (b.ndim - 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("count", [None, 129])
def test_gpu_rk4_sens_fp32_vs_envelope_golden(env, count):
    """sens_fp32 = 1: x+ stays fp64 (1e-12); A, B in fp32 at max(1e-4, 8 x the
    24-bit mpmath error of the same case): operation order and the packed-fma
    tangents on top of the format's own floor at that state."""
    cs, X, U = _rk4_inputs(env, count)
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(sens_fp32=1), 1)
    try:
        xo, A, B = g.rk4_sens(X, U, cs[0]["tf"], cs[0]["M"])
    finally:
        g.close()
    bad = []
    for i in range(len(xo)):
        c = cs[i % len(cs)]
        e = (rel(xo[i], c["xnext"]), rel(A[i], c["A"]), rel(B[i], c["B"]))
        tol = max(FP32_FLOOR, 8 * c["S_err_prec24"])
        if i < len(cs):
            print("fp32 x+ %.2e A %.2e B %.2e bar %.1e %s" % (*e, tol, c["source"]))
        if not (e[0] < bar(c["source"], "xnext") and max(e[1:]) < tol):
            bad.append((i, c["source"], e, tol))
    assert not bad, bad


# ---- B. RTI parity around the orbit ---------------------------------------------

ORBIT_B, ORBIT_OFFSET, ORBIT_STEPS = 16, 7000, 3
EXCLUDE = 1 | 32 | 64       # oracle status bits that take a kite-step out of the parity bars


@functools.lru_cache(maxsize=None)
def oracle_orbit_loop(Nh, wrap):
    """The oracle's closed loop on orbit_batch(16, Nh, 7000): cold step + two
    warm steps, each kite fed the oracle's own plan at node 1.  Per step: the
    inputs (x, and the plan before the step) and the oracle's outputs."""
    kp = ffi.load_params()
    cv = ffi.cfg_vector(ffi.node_config(N=Nh))
    x = orbit_batch(ORBIT_B, Nh, ORBIT_OFFSET)
    if wrap:
        x = wrapped(x)
    Xo = np.zeros((ORBIT_B, Nh + 1, 15)); Uo = np.zeros((ORBIT_B, Nh, 4))
    out = []
    for step in range(ORBIT_STEPS):
        Xin, Uin = Xo.copy(), Uo.copy()
        u0, diag, st = ffi.rti_step(kp, cv, Nh, M, K, x, Xo, Uo, warm=int(step > 0))
        out.append(dict(x=x.copy(), Xin=Xin, Uin=Uin, u0=u0, X=Xo.copy(), U=Uo.copy(), diag=diag, st=st))
        x = Xo[:, 1, :].copy()
    return out


def _excluded(o, step):
    """Kite-steps outside the parity bars: by the oracle's status alone, none
    on the cold step and at most 2 of 16 on a warm step."""
    ex = (o["st"] & EXCLUDE) != 0
    assert ex.sum() <= (0 if step == 0 else 2), (step, o["st"])
    return ex


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("Nh", [20, 40])
def test_oracle_orbit_loop_caps(Nh, wrap):
    """The oracle alone on the inputs of test_gpu_orbit_loop_vs_oracle: the
    exclusion caps hold, the cold step converges, the wrap sets bit 16 on
    exactly kites 8..15 and leaves the plan where it was."""
    from tests.test_gpu_parity import RTI_TOL
    loop = oracle_orbit_loop(Nh, wrap)
    for step, o in enumerate(loop):
        print(Nh, wrap, step, o["st"].tolist(), "kkt max %.1e" % np.nanmax(o["diag"][:, 5]))
        _excluded(o, step)
    st0 = loop[0]["st"]
    assert np.all(np.isfinite(loop[0]["X"]))
    np.testing.assert_array_equal((st0 & 16) != 0, (np.arange(ORBIT_B) >= 8) & wrap)
    if wrap:
        ref = oracle_orbit_loop(Nh, False)
        for a, b in zip(loop, ref):
            ok_ = ((a["st"] | b["st"]) & EXCLUDE) == 0
            # two solves of the same QP up to the rounding of theta -+ 2 pi: RTI_TOL
            assert rel(a["X"][ok_][:, :, :13], b["X"][ok_][:, :, :13]) < RTI_TOL


def test_oracle_lazy_row_resolve_is_not_rounding_driven(kp):
    """Kite 6 of the N = 20 orbit loop at step 2 solves its QP again with four
    state-bound rows (normalised violations up to 4.8) and ends at the cap K
    (residual 2e-9, status bit 8).  While the re-solves used the recursive
    residuals of the first solve, a 1e-15 relative change of this kite-step's
    inputs moved the oracle's own plan by 9.8e-4 (median of 24 seeds, max
    3.0e-3), so no second implementation could meet COND_ENVELOPE there
    (k_qp_tiled: 5.8e-4; k_qp, exact residuals, against the oracle with
    qp_rec = 0: 6.7e-7).  With exact residuals in the re-solves (oracle
    rti_one, k_qp_tiled_lazy) the response is 5.5e-7 (median), 1.7e-6 (max).
    Held to COND_ENVELOPE: the bar the GPU is held to against this oracle
    means something only if the oracle's own rounding response is inside it."""
    from tests.test_gpu_parity import COND_ENVELOPE, rel_per_kite
    Nh, b = 20, 6
    o = oracle_orbit_loop(Nh, False)[2]
    assert o["st"][b] == 8 and o["diag"][b, 5] > 1e-10          # rows bound, QP capped
    cv = ffi.cfg_vector(ffi.node_config(N=Nh))

    def run(Xin, Uin, x):
        X, U = Xin[None].copy(), Uin[None].copy()
        u0, _, _ = ffi.rti_step(kp, cv, Nh, M, K, x[None].copy(), X, U, warm=1)
        return u0, X, U

    ref = run(o["Xin"][b], o["Uin"][b], o["x"][b])
    np.testing.assert_array_equal(ref[1][0], o["X"][b])
    worst = 0.0
    for seed in range(8):
        rng = np.random.default_rng(seed)
        p = lambda a: a * (1 + 1e-15 * rng.normal(size=a.shape))
        got = run(p(o["Xin"][b]), p(o["Uin"][b]), p(o["x"][b]))
        worst = max(worst, max(rel_per_kite(a, c)[0] for a, c in zip(got, ref)))
    print(f"oracle response to a 1e-15 relative input perturbation: {worst:.1e}")
    assert worst < COND_ENVELOPE, worst


def _parity_step(Nh, g, r, o, step):
    from tests.test_gpu_parity import assert_cond_rti, assert_ms_rti, rel_per_kite
    ex = _excluded(o, step)
    keep = ~ex
    # an excluded kite-step still never returns an unflagged non-finite plan
    kkt, its = g.qp_stats()
    print(f"N={Nh} step {step}: gpu status {r['status'].tolist()} iters {its.tolist()} per-kite error",
          ["%.1e" % v for v in np.maximum(rel_per_kite(r["traj"], o["X"]), rel_per_kite(r["ctrl"], o["U"]))])
    fin = np.isfinite(r["traj"]).reshape(ORBIT_B, -1).all(1)
    assert np.all(fin | ((r["status"] & (1 | 32)) != 0)), (step, r["status"])
    if Nh == 20:
        rk = {k: r[k][keep] for k in ("u0", "traj", "ctrl")}
        e = assert_cond_rti(rk, o["u0"][keep], o["X"][keep], o["U"][keep], (Nh, step))
        np.testing.assert_array_equal(r["status"][keep] & ~2, o["st"][keep] & ~2)
    else:
        ek = np.maximum(rel_per_kite(r["traj"][keep], o["X"][keep]), rel_per_kite(r["ctrl"][keep], o["U"][keep]))
        assert_ms_rti(ek, g.qp_stats()[0][keep], o["diag"][keep, 5], (Nh, step))
        np.testing.assert_array_equal(r["status"][keep], o["st"][keep])
        e = float(ek.max(initial=0.0))
    print(f"N={Nh} step {step}: worst kept kite {e:.2e}, gpu status {r['status'].tolist()}")


def _assert_cold_qp(g, kp, Nh, x0):
    """get_qp of every kite after the cold step against ffi.build_qp at the
    bar and the column mapping of test_condensed_qp_vs_oracle."""
    from tests.test_gpu_parity import gpu_to_oracle_perm
    cv = ffi.cfg_vector(dict(ffi.node_config(N=Nh), qp_form=0))
    perm = gpu_to_oracle_perm(Nh)
    for b in range(x0.shape[0]):
        st, X, U, _ = ffi.prologue(kp, cv, Nh, M, x0[b], np.zeros((Nh + 1, 15)), np.zeros((Nh, 4)), warm=0)
        q = ffi.build_qp(kp, cv, Nh, M, X, U)
        gq = g.get_qp(b)
        Hg = np.zeros_like(q["H"]); Hg[np.ix_(perm, perm)] = gq["H"]
        hg = np.zeros_like(q["h"]); hg[perm] = gq["h"]
        assert np.abs(Hg - q["H"]).max() / np.abs(q["H"]).max() < 1e-11, b
        assert np.abs(hg - q["h"]).max() / max(1.0, np.abs(q["h"]).max()) < 1e-11, b
        Cg = np.zeros((Nh, 4 * Nh + 2)); Cg[:, perm] = gq["C"]
        assert np.abs(Cg - q["C"]).max() / max(1.0, np.abs(q["C"]).max()) < 1e-11, b
        np.testing.assert_allclose(gq["cl"], q["c"], rtol=1e-11, atol=1e-11)
        assert np.all(np.isinf(gq["cu"]))


@pytest.mark.gpu
@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("Nh", [20, 40])
def test_gpu_orbit_loop_vs_oracle(kp, Nh, wrap):
    """16 kites around the orbit, cold step + two warm steps, every GPU step
    from the oracle's previous solution (set_solution): N = 20 runs
    k_condense20 + k_qp_tiled with lazy rows, N = 40 the two-wave k_qp_ric.
    With wrap, kites 8..15 enter with theta beyond +-2 pi (status bit 16)."""
    loop = oracle_orbit_loop(Nh, wrap)
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(N=Nh), ORBIT_B)
    try:
        for step, o in enumerate(loop):
            if step > 0:
                g.set_solution(o["Xin"], o["Uin"])
            r = g.step(o["x"])
            if step == 0:
                np.testing.assert_array_equal((r["status"] & 16) != 0, (np.arange(ORBIT_B) >= 8) & wrap)
                np.testing.assert_array_equal((o["st"] & 16) != 0, (np.arange(ORBIT_B) >= 8) & wrap)
                if Nh == 20:
                    _assert_cold_qp(g, kp, Nh, o["x"])
            _parity_step(Nh, g, r, o, step)
    finally:
        g.close()


RESTART_B = 37


@functools.lru_cache(maxsize=None)
def oracle_restart_all(Nh):
    """Cold step of 37 orbit kites, then a plan with one non-finite entry per
    kite.  Offset 7500: the oracle's cold and restarted steps are finite at
    N = 20 and N = 40 there (at 7000 .. 7400 one to three of the phi = 45 deg
    kites go NaN in the oracle's own N = 40 cold step)."""
    kp = ffi.load_params()
    cv = ffi.cfg_vector(ffi.node_config(N=Nh))
    B = RESTART_B
    x = orbit_batch(B, Nh, 7500)
    Xo = np.zeros((B, Nh + 1, 15)); Uo = np.zeros((B, Nh, 4))
    u0, diag, st = ffi.rti_step(kp, cv, Nh, M, K, x, Xo, Uo, warm=0)
    cold = dict(x=x, u0=u0, X=Xo.copy(), U=Uo.copy(), diag=diag, st=st)
    x1 = Xo[:, 1, :].copy()
    for b in range(B):
        if b % 3 == 2:
            Uo[b, b % Nh, b % 4] = np.nan
        else:
            Xo[b, 2 + b % (Nh - 1), b % 15] = np.nan if b % 3 else np.inf
    Xin, Uin = Xo.copy(), Uo.copy()
    u0, diag, st = ffi.rti_step(kp, cv, Nh, M, K, x1, Xo, Uo, warm=1)
    return cold, dict(x=x1, Xin=Xin, Uin=Uin, u0=u0, X=Xo.copy(), U=Uo.copy(), diag=diag, st=st)


@pytest.mark.parametrize("Nh", [20, 40])
def test_oracle_every_kite_restarts(Nh):
    cold, o = oracle_restart_all(Nh)
    print(Nh, cold["st"].tolist(), o["st"].tolist())
    assert np.all(o["st"] & 64) and not np.any(o["st"] & 1) and np.all(np.isfinite(o["X"]))


@pytest.mark.gpu
@pytest.mark.parametrize("Nh", [20, 40])
def test_gpu_every_kite_restarts_vs_oracle(Nh):
    """All 37 kites of the batch restart cold in one warm step (non-finite
    injected plan): the whole batch through k_prologue_warm's cold list and
    k_prologue_cold's grid-stride loop; bit 64 everywhere and oracle parity."""
    from tests.test_gpu_parity import assert_cond_rti, assert_ms_rti, rel_per_kite
    cold, o = oracle_restart_all(Nh)
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(N=Nh), RESTART_B)
    try:
        g.step(cold["x"])
        g.set_solution(o["Xin"], o["Uin"])
        r = g.step(o["x"])
        kkt = g.qp_stats()[0]
    finally:
        g.close()
    assert np.all(r["status"] & 64) and np.all(o["st"] & 64)
    assert np.all(np.isfinite(r["traj"]))
    if Nh == 20:
        assert_cond_rti(r, o["u0"], o["X"], o["U"], Nh)
        np.testing.assert_array_equal(r["status"] & ~2, o["st"] & ~2)
    else:
        e = np.maximum(rel_per_kite(r["traj"], o["X"]), rel_per_kite(r["ctrl"], o["U"]))
        assert_ms_rti(e, kkt, o["diag"][:, 5], Nh)
        np.testing.assert_array_equal(r["status"], o["st"])


# ---- C. batch-position invariance, bitwise ----------------------------------------

def _closed_loop(Nh, x0, wind, steps=3):
    """Three closed-loop steps, each kite fed its own traj[:, 1]."""
    B = x0.shape[0]
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(N=Nh), B)
    out = []
    try:
        if wind is not None:
            g.set_wind(wind)
        x = x0.copy()
        for _ in range(steps):
            r = g.step(x)
            kkt, it = g.qp_stats()
            out.append(dict(u0=r["u0"].copy(), traj=r["traj"].copy(), ctrl=r["ctrl"].copy(),
                            status=r["status"].copy(), kkt=kkt.copy(), iters=it.copy()))
            x = r["traj"][:, 1, :].copy()
    finally:
        g.close()
    return out


def _assert_same(ref, got, sel, what):
    for step, (a, b) in enumerate(zip(ref, got)):
        for k in a:
            np.testing.assert_array_equal(a[k][sel], b[k], err_msg=f"{what}: {k}, step {step}")


@pytest.mark.gpu
@pytest.mark.parametrize("windy", [True, False])
@pytest.mark.parametrize("Nh", [20, 40])
def test_gpu_batch_position_invariance(Nh, windy):
    """A kite's result does not depend on where it sits in the batch, nor on
    who else is in it: u0, traj, ctrl, status and qp_stats bitwise equal for
    the natural order, a seeded permutation, the interior shard 13..28 and
    (with wind) the tail kite alone.  The orbit kites take unequal iteration
    counts, so k_qp_order reorders them on the warm steps.  No oracle and no
    tolerance: a difference is a cross-kite dependence or an indexing error."""
    from tests.test_wind import winds
    B = 37
    x0 = orbit_batch(B, Nh, 7100)
    wd = winds(B, seed=71) if windy else None
    sub = lambda idx: None if wd is None else wd[idx]
    nat = _closed_loop(Nh, x0, wd)
    its = np.concatenate([o["iters"] for o in nat[:-1]])
    assert len(set(its.tolist())) > 1, its          # the warm-step reorder has something to reorder
    perm = np.random.default_rng(37).permutation(B)
    assert not np.array_equal(perm, np.arange(B))
    got = _closed_loop(Nh, x0[perm], sub(perm))      # got[i] is kite perm[i]
    _assert_same(nat, got, perm, "permuted")
    sl = np.arange(13, 29)
    _assert_same(nat, _closed_loop(Nh, x0[sl], sub(sl)), sl, "shard 13..28")
    if windy:
        _assert_same(nat, _closed_loop(Nh, x0[36:], sub(slice(36, None))), slice(36, None), "kite 36 alone")


# ---- D. k_ekf: partial blocks and envelope states -----------------------------------

def _assert_ekf_vs_oracle(kp, xg, Pg, x, u, P, z, W, V, dt, what):
    for b in range(x.shape[0]):
        xo, Po = ffi.ekf_step(kp, x[b], u[b], dt, P[b], None if z is None else z[b], W, V)
        np.testing.assert_allclose(xg[b], xo, rtol=1e-12, atol=1e-13, err_msg=f"{what} kite {b}")
        np.testing.assert_allclose(Pg[b], Po, rtol=1e-11, atol=1e-13, err_msg=f"{what} kite {b}")


@pytest.mark.gpu
@pytest.mark.parametrize("update", [False, True])
def test_gpu_ekf_partial_blocks(ctx1, kp, update):
    """k_ekf packs 4 kites per block: counts 1, 5, 6, 7 leave 1..3 lanes groups
    of the last block without a kite.  Each against the oracle, and bitwise
    equal to the same kites inside a count-8 call."""
    from tests.test_ekf import _inputs
    x, u, P, z, W, V = _inputs(8)
    dt = 0.02
    zz = z if update else None
    x8, P8 = ctx1.ekf_step(x, u, P, dt, zz, W, V)
    _assert_ekf_vs_oracle(kp, x8, P8, x, u, P, zz, W, V, dt, "count 8")
    for c in (1, 5, 6, 7):
        xc, Pc = ctx1.ekf_step(x[:c], u[:c], P[:c], dt, None if zz is None else zz[:c], W, V)
        _assert_ekf_vs_oracle(kp, xc, Pc, x[:c], u[:c], P[:c], None if zz is None else zz[:c], W, V, dt, f"count {c}")
        np.testing.assert_array_equal(xc, x8[:c])
        np.testing.assert_array_equal(Pc, P8[:c])


@pytest.mark.gpu
@pytest.mark.parametrize("update", [False, True])
def test_gpu_ekf_envelope_states(ctx1, kp, env, update):
    """k_ekf at the fixture's orbit, attitude, tether and sideslip states with
    the seeded SPD covariances and measurement noise of test_ekf._inputs."""
    from tests.test_ekf import _inputs
    cs = [c for c in env["rhs"] if regime(c["source"]) in ("orbit", "attitude", "tether", "sideslip")]
    B = len(cs)
    xs, _, P, zs, W, V = _inputs(B)
    x = np.array([c["x"] for c in cs]); u = np.array([c["u"] for c in cs])
    z = x[:, 6:13] + (zs - xs[:, 6:13])
    zz = z if update else None
    xg, Pg = ctx1.ekf_step(x, u, P, 0.02, zz, W, V)
    _assert_ekf_vs_oracle(kp, xg, Pg, x, u, P, zz, W, V, 0.02, "envelope")
