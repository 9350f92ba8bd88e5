"""GPU tests of the closed-loop scorer (score_kernels.hip: k_closest_global,
k_score, k_score_summary) through the C ABI, the Python binding and the fleet
loop, against the float64 reference tests/score_ref.py.

Bars.  tests/test_score_ref.py::test_rounding_envelope measures, on the CPU and
from the reference alone, the worst |float64 reference - 50-digit value| of
each per-period quantity over exactly the inputs used here (174 periods); the
bar of a quantity is 32 times that envelope (score_ref.ENVELOPE, BAR_FACTOR):

    quantity   envelope    bar (32 x)
    theta*     4.4e-16     1.41e-14  rad
    d          1.2e-15     3.84e-14  m
    d^2        8.8e-16     2.82e-14  m^2
    l_track    1.2e-12     3.84e-11  (controller units, values up to 1e3)
    l_u        4.4e-17     1.41e-15
    rate       2.0e-15     6.40e-14
    ||v||      1.1e-15     3.52e-14  m/s
    dtheta     9.3e-16     2.98e-14  rad (one progress step)

A slot that sums a quantity over n periods has n times its bar; max d and min
||v|| have the bar of d and ||v||; integer-valued slots are exact.  The fleet
summary is compared with math.fsum of the same rows: the bar is the bound of
any summation order of B terms, B 2^-53 sum|x|.  Every other comparison here is
bitwise (host against device entry point, batch shape and position, loop
against hand calls).

Batch shapes 1, 3, 4, 5, 9: around the four-kites-per-block boundary."""
import math

import numpy as np
import pytest
import torch

import openkite_amd as ok
from openkite_amd import nmpc
from openkite_amd.fleet import EpisodeScore, FleetLoop, GpuPlant, GpuStepper
from tests import score_ref as sr
from tests.test_path import fourier_path, product_config

pytestmark = pytest.mark.gpu

SHAPES = [1, 3, 4, 5, 9]
SUM_SLOTS = {sr.SUM_D2: "d2", sr.SUM_TRACK: "track", sr.SUM_U: "u", sr.SUM_SPEED: "speed"}
RATE_SLOTS = {sr.SUM_RATE: "rate", sr.PROGRESS: "dtheta"}


def cfg_of(kind):
    return ok.default_config() if kind == "circle" else product_config(fourier_path())


@pytest.fixture(scope="module")
def ctxs():
    """One context per path (batch 4: `count` need not be the batch)."""
    out = {k: ok.BatchNMPC(ok.load_properties(), cfg_of(k), 4) for k in ("circle", "fourier")}
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def consts():
    return {k: sr.consts(cfg_of(k)) for k in ("circle", "fourier")}


@pytest.fixture(scope="module")
def episodes(consts):
    """Per path: the inputs and the reference rows after every period (computed once)."""
    out = {}
    for kind, C in consts.items():
        x, u, st, ps = sr.episode_inputs(C, sr.EP_B, sr.EP_T, sr.EP_SEED[kind])
        acc, mem = np.zeros((sr.EP_B, 16)), np.zeros((sr.EP_B, 8))
        hist = []
        for t in range(sr.EP_T):
            sr.score_batch(C, x[t], u[t], st[t], ps[t], t == 0, acc, mem)
            hist.append((acc.copy(), mem.copy()))
        for a in (x, u, st, ps):
            a.setflags(write=False)
        out[kind] = dict(x=x, u=u, st=st, ps=ps, hist=hist)
    return out


def run_host(g, ep, B, T=sr.EP_T, cols=None):
    cols = np.arange(B) if cols is None else np.asarray(cols)
    acc, mem = np.zeros((len(cols), 16)), np.zeros((len(cols), 8))
    for t in range(T):
        g.score_step(ep["x"][t, cols], ep["u"][t, cols], acc, mem, ep["st"][t, cols], ep["ps"][t, cols], first=t == 0)
    return acc, mem


def check_rows(acc, mem, ref_acc, ref_mem, what):
    for b in range(acc.shape[0]):
        a, r = acc[b], ref_acc[b]
        for k in sr.INT_SLOTS:
            assert a[k] == r[k], (what, b, k, a[k], r[k])
        n, nr = r[sr.N], r[sr.N_RATE]
        for k, q in SUM_SLOTS.items():
            print(f"{what} kite {b} slot {k}: |gpu - ref| = {abs(a[k] - r[k]):.3e}  bar {n * sr.bar(q):.3e}")
            assert abs(a[k] - r[k]) <= n * sr.bar(q), (what, b, k, a[k], r[k])
        for k, q in RATE_SLOTS.items():
            print(f"{what} kite {b} slot {k}: |gpu - ref| = {abs(a[k] - r[k]):.3e}  bar {nr * sr.bar(q):.3e}")
            assert abs(a[k] - r[k]) <= nr * sr.bar(q), (what, b, k, a[k], r[k])
        assert abs(a[sr.MAX_D] - r[sr.MAX_D]) <= sr.bar("d"), (what, b)
        assert abs(a[sr.MIN_SPEED] - r[sr.MIN_SPEED]) <= sr.bar("speed"), (what, b)
        m, rm = mem[b], ref_mem[b]
        assert m[sr.MEM_VALID] == rm[sr.MEM_VALID] and np.array_equal(m[6:], rm[6:]), (what, b)
        if n > 0:
            assert abs(m[sr.MEM_THETA] - rm[sr.MEM_THETA]) <= sr.bar("theta"), (what, b)
            np.testing.assert_array_equal(m[sr.MEM_U:sr.MEM_U + 4], rm[sr.MEM_U:sr.MEM_U + 4])


# ---- 1. the global closest point ------------------------------------------------
@pytest.mark.parametrize("kind", ["circle", "fourier"])
def test_closest_point_global_vs_reference(ctxs, consts, kind):
    g, C = ctxs[kind], consts[kind]
    pos = sr.positions(C, 22, sr.CP_SEED[kind])
    ref = [sr.closest_point(C, r)[:2] for r in pos]
    for B in SHAPES:
        lo, hi = sr.CP_SLICES[B]
        th, d = g.closest_point_global(pos[lo:hi])
        assert th.shape == (B,) and d.shape == (B,)
        for i in range(B):
            rt, rd = ref[lo + i]
            print(f"{kind} B={B} i={i}: |dtheta| {abs(th[i] - rt):.3e} |dd| {abs(d[i] - rd):.3e}")
            assert abs(th[i] - rt) <= sr.bar("theta") and abs(d[i] - rd) <= sr.bar("d"), (kind, B, i)
            assert -2 * math.pi / 64 <= th[i] < 2 * math.pi
            if (lo + i) % 10 == 0:
                assert d[i] <= sr.bar("d")             # exactly on the path
    # a non-finite position: NaN for that kite alone
    bad = pos[:5].copy()
    bad[1, 2] = np.nan; bad[4, 0] = np.inf
    th, d = g.closest_point_global(bad)
    good, _ = g.closest_point_global(pos[:5])
    assert np.isnan(th[[1, 4]]).all() and np.isnan(d[[1, 4]]).all()
    np.testing.assert_array_equal(th[[0, 2, 3]], good[[0, 2, 3]])
    # the device entry point, on torch's stream
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        p = torch.from_numpy(pos[:9].copy()).cuda()
        t = torch.zeros(9, dtype=torch.float64, device="cuda"); dd = torch.zeros_like(t)
        g.closest_point_global_device(9, p.data_ptr(), t.data_ptr(), dd.data_ptr())
        torch.cuda.synchronize()
        th9, d9 = g.closest_point_global(pos[:9])
        np.testing.assert_array_equal(t.cpu().numpy(), th9)
        np.testing.assert_array_equal(dd.cpu().numpy(), d9)
    finally:
        g.use_own_stream()


# ---- 2. score_step against the reference, and its bitwise properties ---------------
@pytest.mark.parametrize("kind", ["circle", "fourier"])
def test_score_step_vs_reference(ctxs, episodes, kind):
    g, ep = ctxs[kind], episodes[kind]
    rows = {}
    for B in SHAPES:
        acc, mem = run_host(g, ep, B)
        check_rows(acc, mem, ep["hist"][-1][0][:B], ep["hist"][-1][1][:B], f"{kind} B={B}")
        rows[B] = (acc, mem)
    # rows 0..3 of the B = 5 run == the B = 4 run; and every smaller batch is a prefix of B = 9
    np.testing.assert_array_equal(rows[5][0][:4], rows[4][0])
    np.testing.assert_array_equal(rows[5][1][:4], rows[4][1])
    for B in SHAPES:
        np.testing.assert_array_equal(rows[9][0][:B], rows[B][0])
    # a kite's row does not depend on its place in the batch
    perm = np.array([5, 0, 8, 3, 1, 7, 2, 6, 4])
    pa, pm = run_host(g, ep, 9, cols=perm)
    np.testing.assert_array_equal(pa, rows[9][0][perm])
    np.testing.assert_array_equal(pm, rows[9][1][perm])
    # the lost kites of the inputs were lost, the others were not
    assert rows[9][0][0, sr.N_LOST] == 1 and rows[9][0][8, sr.N_LOST] == 1 and rows[9][0][1:8, sr.N_LOST].sum() == 0


@pytest.mark.parametrize("B", SHAPES)
def test_score_step_host_equals_device(ctxs, episodes, B):
    g, ep = ctxs["circle"], episodes["circle"]
    want_acc, want_mem = run_host(g, ep, B)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        acc = torch.zeros((B, 16), dtype=torch.float64, device="cuda"); mem = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
        stepper = GpuStepper(g)
        for t in range(sr.EP_T):
            x = torch.from_numpy(ep["x"][t, :B].copy()).cuda(); u = torch.from_numpy(ep["u"][t, :B].copy()).cuda()
            st = torch.from_numpy(ep["st"][t, :B].copy()).cuda(); ps = torch.from_numpy(ep["ps"][t, :B].copy()).cuda()
            stepper.score(x, u, st, ps, t == 0, acc, mem)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(acc.cpu().numpy(), want_acc)
        np.testing.assert_array_equal(mem.cpu().numpy(), want_mem)
        # the status words are optional
        a2 = torch.zeros_like(acc); m2 = torch.zeros_like(mem)
        stepper.score(x, u, None, None, True, a2, m2)
        torch.cuda.synchronize()
        assert (a2[:, sr.N] == 1).all() and (a2[:, sr.N_LOST] == 0).all()
    finally:
        g.use_own_stream()


# ---- 3. a lost period is contained ---------------------------------------------------
def test_lost_periods_are_contained(ctxs, episodes):
    g, ep = ctxs["circle"], episodes["circle"]
    B = 5
    zero = np.zeros(B, dtype=np.int32)
    acc0, mem0 = np.zeros((B, 16)), np.zeros((B, 8))
    for t in (0, 1):
        g.score_step(ep["x"][t, :B], ep["u"][t, :B], acc0, mem0, zero, zero, first=t == 0)
    x3, u3, x4, u4 = ep["x"][3, :B], ep["u"][3, :B], ep["x"][4, :B], ep["u"][4, :B]
    clean_a, clean_m = g.score_step(x3, u3, acc0.copy(), mem0.copy(), zero, zero)
    assert (clean_a[:, sr.N] == 3).all() and (clean_a[:, sr.N_RATE] == 2).all()
    keep = [k for k in range(16) if k not in (sr.N_LOST, sr.EVER_LOST)]
    cases = [("x", np.nan, 0, 0), ("x", -np.inf, 0, 0), ("u", np.nan, 0, 0), ("ps", 0, 0, nmpc.PLANT_NAN),
             ("st", 0, nmpc.ST_NAN, 0), ("st", 0, nmpc.ST_STEP_REJECTED, 0),
             ("st", 0, nmpc.ST_RESTART | nmpc.ST_MIN_SPEED, 0)]
    for kite in (1, 4):                                # inside the first block, alone in the second
        for i, (what, v, sbit, pbit) in enumerate(cases):
            x, u, st, ps = x3.copy(), u3.copy(), zero.copy(), zero.copy()
            if what == "x":
                x[kite, (i * 5) % 13] = v
            elif what == "u":
                u[kite, 2] = v
            st[kite] |= sbit
            ps[kite] |= pbit
            a, m = g.score_step(x, u, acc0.copy(), mem0.copy(), st, ps)
            assert a[kite, sr.N_LOST] == 1 and a[kite, sr.EVER_LOST] == 1 and m[kite, sr.MEM_VALID] == 0, (kite, i)
            np.testing.assert_array_equal(a[kite, keep], acc0[kite, keep])
            np.testing.assert_array_equal(m[kite, :5], mem0[kite, :5])
            others = [b for b in range(B) if b != kite]
            np.testing.assert_array_equal(a[others], clean_a[others])
            np.testing.assert_array_equal(m[others], clean_m[others])
            # the period after the lost one: scored, but no rate and no progress
            b4, _ = g.score_step(x4, u4, a.copy(), m.copy(), zero, zero)
            assert b4[kite, sr.N] == 3 and b4[kite, sr.N_RATE] == 1 and b4[kite, sr.N_LOST] == 1
            assert b4[kite, sr.SUM_RATE] == acc0[kite, sr.SUM_RATE] and b4[kite, sr.PROGRESS] == acc0[kite, sr.PROGRESS]
            assert (b4[others, sr.N_RATE] == 3).all()


# ---- 4. first, the wrap and a whole lap -----------------------------------------------
@pytest.mark.parametrize("direction", [1, -1])
def test_first_and_a_lap_across_two_pi(ctxs, consts, direction):
    g, C = ctxs["circle"], consts["circle"]
    x, u = sr.lap_inputs(C, direction)
    acc, mem = np.zeros((1, 16)), np.zeros((1, 8))
    ra, rm = np.zeros(16), np.zeros(8)
    for k in range(13):
        g.score_step(x[k:k + 1], u[k:k + 1], acc, mem, first=k == 0)
        sr.score_step(C, x[k], u[k], 0, 0, k == 0, ra, rm)
        if k == 0:
            assert acc[0, sr.N] == 1 and acc[0, sr.N_RATE] == 0 and acc[0, sr.PROGRESS] == 0 and acc[0, sr.SUM_RATE] == 0
    check_rows(acc, mem, ra[None], rm[None], f"lap {direction}")
    print(f"lap {direction}: progress {acc[0, sr.PROGRESS]!r}, off 2 pi by {abs(acc[0, sr.PROGRESS] - direction * 2 * math.pi):.3e}")
    assert acc[0, sr.N_RATE] == 12
    assert abs(acc[0, sr.PROGRESS] - direction * 2 * math.pi) <= 12 * sr.bar("dtheta")
    # first = 1 mid-flight: scored, no rate, no progress
    before = acc.copy()
    g.score_step(x[5:6], u[5:6], acc, mem, first=True)
    assert acc[0, sr.N] == 14 and acc[0, sr.N_RATE] == 12
    assert acc[0, sr.PROGRESS] == before[0, sr.PROGRESS] and acc[0, sr.SUM_RATE] == before[0, sr.SUM_RATE]


# ---- 5. status counts, and min / max from an all-zero row -----------------------------
def test_status_counts_and_min_max_from_reset(ctxs, consts, episodes):
    g, C, ep = ctxs["circle"], consts["circle"], episodes["circle"]
    acc, mem = run_host(g, ep, 9)
    st, ps = ep["st"], ep["ps"]
    scored = ((st & sr.LOSING) == 0) & ((ps & sr.PLANT_NAN) == 0)
    for slot, bit in ((sr.N_MIN_SPEED, nmpc.ST_MIN_SPEED), (sr.N_QP_NOT_CONV, nmpc.ST_QP_NOT_CONV),
                      (sr.N_STATE_BOUND, nmpc.ST_STATE_BOUND)):
        want = (((st & bit) != 0) & scored).sum(axis=0)
        np.testing.assert_array_equal(acc[:, slot], want)
        assert want.sum() > 0
    np.testing.assert_array_equal(acc[:, sr.N], scored.sum(axis=0))
    # one period from all-zero rows: the max and the min are that period's values, not 0
    a1, _ = run_host(g, ep, 9, T=1)
    for b in range(9):
        q = sr.period(C, ep["x"][0, b], ep["u"][0, b], np.zeros(8), True)
        assert abs(a1[b, sr.MAX_D] - q["d"]) <= sr.bar("d") and abs(a1[b, sr.MIN_SPEED] - q["speed"]) <= sr.bar("speed")
        assert a1[b, sr.MIN_SPEED] > 1.0 and (b % 10 == 0 or a1[b, sr.MAX_D] > 0)
        assert a1[b, sr.SUM_D2] == a1[b, sr.MAX_D] * a1[b, sr.MAX_D] and a1[b, sr.SUM_SPEED] == a1[b, sr.MIN_SPEED]


# ---- 6. the fleet summary ---------------------------------------------------------------
@pytest.mark.parametrize("B", [9, 300])
def test_score_summary_vs_fsum(ctxs, episodes, B):
    g = ctxs["circle"]
    ref = episodes["circle"]["hist"][-1][0]
    acc = np.zeros((B, 16))
    for i in range(B):
        acc[i] = ref[i % 9]
        for k in range(16):
            if k not in sr.INT_SLOTS:
                acc[i, k] *= 1.0 + i / 1024.0
    if B > 9:
        acc[[17, 256, 299]] = 0.0                       # kites never scored: no part in max / min
        acc[256, sr.N_LOST] = 6.0; acc[256, sr.EVER_LOST] = 1.0
    want = sr.summary(acc)
    got = g.score_summary(acc)
    for k in range(16):
        if k in sr.INT_SLOTS or k in (sr.MAX_D, sr.MIN_SPEED, sr.KITES):
            assert got[k] == want[k], (k, got[k], want[k])
        else:
            bound = B * 2.0 ** -53 * np.abs(acc[:, k]).sum()
            print(f"B={B} slot {k}: |gpu - fsum| = {abs(got[k] - want[k]):.3e}  bound {bound:.3e}")
            assert abs(got[k] - want[k]) <= bound, (k, got[k], want[k])
    assert got[sr.KITES] == B and got[sr.MIN_SPEED] > 0
    np.testing.assert_array_equal(g.score_summary(acc), got)            # reproducible
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        a = torch.from_numpy(acc).cuda(); out = torch.zeros(16, dtype=torch.float64, device="cuda")
        GpuStepper(g).score_summary(a, out)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), got)
    finally:
        g.use_own_stream()
    # all rows unscored: no max, no min
    z = g.score_summary(np.zeros((5, 16)))
    assert z[sr.KITES] == 5 and not z[:15].any()


# ---- 7. the fleet loop ------------------------------------------------------------------
def test_fleet_loop_scores_on_the_stream():
    from bench import synthetic_x0
    nk, Nh, steps, restart_at = 8, 20, 12, 8
    cfg = ok.default_config(N=Nh)
    h, psteps, sub = cfg.dt / 2, 2, 5
    P = ok.perturb_params(ok.load_properties(), nk, 0.1, seed=23)
    scored = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    plain = ok.BatchNMPC(ok.load_properties(), cfg, nk)
    try:
        for c in (scored, plain):
            c.plant_set_params(P)
            c.set_stream(torch.cuda.current_stream().cuda_stream)
        x_init = torch.from_numpy(synthetic_x0(nk, 0, scored)).cuda()
        with pytest.raises(ValueError):
            FleetLoop(GpuStepper(scored), x_init, Nh, cfg.dt, plant=GpuPlant(scored, h, psteps, sub),
                      scorer=EpisodeScore(nk - 1, device="cuda"))
        score = EpisodeScore(nk, device="cuda")
        loop = FleetLoop(GpuStepper(scored), x_init, Nh, cfg.dt, plant=GpuPlant(scored, h, psteps, sub), scorer=score)
        ref = FleetLoop(GpuStepper(plain), x_init, Nh, cfg.dt, plant=GpuPlant(plain, h, psteps, sub))
        acc, mem = np.zeros((nk, 16)), np.zeros((nk, 8))
        first = True
        for s in range(steps):
            if s == restart_at:
                loop.restart(); ref.restart()
                first = True
                assert score.first
            xp, ps = loop.xp.cpu().numpy().copy(), loop.plant_status.cpu().numpy().copy()
            n_rate = score.acc[:, sr.N_RATE].cpu().numpy().copy()
            loop.step(); ref.step()
            torch.cuda.synchronize()
            for name in ("u0", "traj", "status"):
                np.testing.assert_array_equal(getattr(loop, name).cpu().numpy(), getattr(ref, name).cpu().numpy(),
                                              err_msg=f"{name} step {s}")
            scored.score_step(xp, loop.u0.cpu().numpy(), acc, mem, loop.status.cpu().numpy(), ps, first=first)
            np.testing.assert_array_equal(score.acc.cpu().numpy(), acc, err_msg=f"acc step {s}")
            np.testing.assert_array_equal(score.mem.cpu().numpy(), mem, err_msg=f"mem step {s}")
            if first:                                  # no rate, no progress; n keeps counting
                np.testing.assert_array_equal(score.acc[:, sr.N_RATE].cpu().numpy(), n_rate)
            first = False
            assert not score.first
        rows = score.rows()
        assert set(rows) == set(nmpc.SCORE_SLOTS)
        n = rows["n"].cpu().numpy() + rows["n_lost"].cpu().numpy()
        np.testing.assert_array_equal(n, np.full(nk, steps))
        assert rows["n"].sum().item() > 0
        summ = score.summary()
        np.testing.assert_array_equal(np.array(summ["raw"]), scored.score_summary(acc))
        assert summ["kites"] == nk and summ["n"] + summ["n_lost"] == nk * steps
        assert math.isfinite(summ["rms_d"]) and summ["rms_d"] > 0 and summ["rms_d"] <= summ["max_d"]
        assert EpisodeScore.combine([summ["raw"], summ["raw"]])["n"] == 2 * summ["n"]
        score.reset()
        assert not score.acc.any() and not score.mem.any() and score.first
    finally:
        scored.close()
        plain.close()
