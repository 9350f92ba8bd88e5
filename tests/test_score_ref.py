"""CPU tests of the scorer's float64 reference (tests/score_ref.py), and the
measurement of its rounding envelope.

The reference is checked against a brute force (200 000 samples of theta and an
unclamped Newton refinement) on the node's circle and on the three-harmonic
path of tests/test_path.py, on positions exactly on the path, across the wrap
at 2 pi, and through the lost rule, ``first``, the summary and ``combine``.

test_rounding_envelope evaluates every per-period quantity of every input the
GPU tests use (score_ref.gpu_test_inputs) twice, in float64 and in mpmath at 50
digits, and prints the worst difference per quantity.  Those figures, taken
from the reference alone, are recorded in score_ref.ENVELOPE; the GPU bars of
tests/test_score.py are 32 times them.

Input condition, asserted here for every position used: within 1.5 m of the
path, at least 0.5 m from the circle's axis, and the best two local minima of
the distance at least 1e-3 m apart -- the global closest point is then
unambiguous."""
import math

import numpy as np
import pytest

import openkite_amd as ok
from tests import score_ref as sr
from tests.test_path import fourier_path, product_config


def cfg_of(kind):
    return ok.default_config() if kind == "circle" else product_config(fourier_path())


@pytest.fixture(scope="module", params=["circle", "fourier"])
def C(request):
    return sr.consts(cfg_of(request.param))


def test_consts_are_the_node_configuration():
    C = sr.consts(ok.default_config())
    assert C["K"] == 0 and C["R"] == 2.65 and len(C["Q"]) == 3 and len(C["Rw"]) == 4
    F = sr.consts(product_config(fourier_path()))
    assert F["K"] == 3 and F["F"][1, 6] == -0.2


def test_path_derivatives(C):
    th = np.linspace(-0.2, 6.4, 41)
    P, dP, ddP = sr.path_np(C, th)
    for i, t in enumerate(th):                       # the scalar recurrence == the direct form
        p, d, dd = sr.path(C, float(t))
        np.testing.assert_allclose(p, P[:, i], rtol=0, atol=5e-15)
        np.testing.assert_allclose(d, dP[:, i], rtol=0, atol=2e-14)
        np.testing.assert_allclose(dd, ddP[:, i], rtol=0, atol=5e-14)
    h = 1e-5
    Pp, dPp, _ = sr.path_np(C, th + h)
    Pm, dPm, _ = sr.path_np(C, th - h)
    np.testing.assert_allclose((Pp - Pm) / (2 * h), dP, rtol=0, atol=1e-8)
    np.testing.assert_allclose((dPp - dPm) / (2 * h), ddP, rtol=0, atol=1e-7)
    Pc, dPc = ok.path_eval(cfg_of("circle" if C["K"] == 0 else "fourier"), th)   # the product's host path
    np.testing.assert_allclose(P.T, Pc, rtol=0, atol=5e-15)
    np.testing.assert_allclose(dP.T, dPc, rtol=0, atol=2e-14)


def test_closest_point_against_brute_force(C):
    pos = sr.positions(C, 40, seed=3)
    worst_d = worst_th = 0.0
    for i, r in enumerate(pos):
        assert sr.condition_ok(C, r), i
        th, d, _ = sr.closest_point(C, r)
        tb, db = sr.brute_force(C, r)
        assert -2 * math.pi / 64 <= th < 2 * math.pi
        worst_d = max(worst_d, abs(d - db))
        worst_th = max(worst_th, abs(sr.wrap(th - tb)))
        if i % 10 == 0:
            assert d < 1e-15, (i, d)                 # exactly on the path
    print(f"closest point vs brute force (K = {C['K']}): worst |dd| {worst_d:.2e}, worst |dtheta| {worst_th:.2e}")
    assert worst_d < 5e-15 and worst_th < 5e-14


def test_closest_point_edges(C):
    th, d, _ = sr.closest_point(C, [math.nan, 0.0, 1.0])
    assert math.isnan(th) and math.isnan(d)
    th, d, _ = sr.closest_point(C, [1.0, math.inf, 1.0])
    assert math.isnan(th) and math.isnan(d)
    # a point of the path just below 2 pi and just above 0: the nearest sample is
    # 63 or 0, theta* stays in [-2 pi / 64, 2 pi)
    for t in (2 * math.pi - 1e-3, 1e-3, 0.0):
        th, d, _ = sr.closest_point(C, sr.path(C, t)[0])
        assert abs(sr.wrap(th - t)) < 1e-14 and d < 1e-15 and -2 * math.pi / 64 <= th < 2 * math.pi


def test_wrap():
    assert sr.wrap(math.pi) == math.pi and sr.wrap(-math.pi) == math.pi
    assert sr.wrap(3.5) == 3.5 - 2 * math.pi and sr.wrap(-3.5) == -3.5 + 2 * math.pi and sr.wrap(0.25) == 0.25


def test_lap_progress_and_first():
    C = sr.consts(ok.default_config())
    for direction in (1, -1):
        x, u = sr.lap_inputs(C, direction)
        acc, mem = np.zeros(16), np.zeros(8)
        for k in range(13):
            sr.score_step(C, x[k], u[k], 0, 0, k == 0, acc, mem)
            if k == 0:
                assert acc[sr.PROGRESS] == 0.0 and acc[sr.SUM_RATE] == 0.0 and acc[sr.N_RATE] == 0.0
        assert acc[sr.N] == 13 and acc[sr.N_RATE] == 12 and acc[sr.N_LOST] == 0
        assert abs(acc[sr.PROGRESS] - direction * 2 * math.pi) < 1e-13
        assert acc[sr.MAX_D] < 4e-15 and acc[sr.MIN_SPEED] == math.sqrt(16.0 + 0.0625 + 0.25)
        # first again: the accumulators go on, the period has no predecessor
        before = acc.copy()
        sr.score_step(C, x[3], u[3], 0, 0, True, acc, mem)
        assert acc[sr.N] == 14 and acc[sr.PROGRESS] == before[sr.PROGRESS] and acc[sr.SUM_RATE] == before[sr.SUM_RATE]


def test_lost_rule_and_reset_rows():
    C = sr.consts(ok.default_config())
    x, u, st, ps = sr.episode_inputs(C, 2, 4, seed=5)
    st[:] = 0; ps[:] = 0
    acc, mem = np.zeros(16), np.zeros(8)               # all-zero rows are a valid reset
    sr.score_step(C, x[0, 0], u[0, 0], sr.ST_MIN_SPEED | sr.ST_THETA_WRAP, 0, True, acc, mem)
    sr.score_step(C, x[1, 0], u[1, 0], sr.ST_QP_NOT_CONV | sr.ST_STATE_BOUND, 0, False, acc, mem)
    assert acc[sr.N] == 2 and acc[sr.N_RATE] == 1 and mem[sr.MEM_VALID] == 1
    assert (acc[sr.N_MIN_SPEED], acc[sr.N_QP_NOT_CONV], acc[sr.N_STATE_BOUND]) == (1, 1, 1)
    assert acc[sr.MAX_D] > 0 and acc[sr.MIN_SPEED] > 0 and acc[sr.SPARE] == 0
    xn = x[2, 0].copy(); xn[4] = math.nan
    un = u[2, 0].copy(); un[3] = math.inf
    cases = [(xn, u[2, 0], 0, 0), (x[2, 0], un, 0, 0), (x[2, 0], u[2, 0], 0, sr.PLANT_NAN),
             (x[2, 0], u[2, 0], sr.ST_NAN, 0), (x[2, 0], u[2, 0], sr.ST_STEP_REJECTED, 0),
             (x[2, 0], u[2, 0], sr.ST_RESTART | sr.ST_MIN_SPEED, 0)]
    for xx, uu, s, p in cases:
        a, m = acc.copy(), mem.copy()
        sr.score_step(C, xx, uu, s, p, False, a, m)
        assert a[sr.N_LOST] == 1 and a[sr.EVER_LOST] == 1 and m[sr.MEM_VALID] == 0
        keep = [k for k in range(16) if k not in (sr.N_LOST, sr.EVER_LOST)]
        np.testing.assert_array_equal(a[keep], acc[keep])
        np.testing.assert_array_equal(m[:5], mem[:5])
        b = a.copy()                                   # the period after a lost one: no rate, no progress
        sr.score_step(C, x[3, 0], u[3, 0], 0, 0, False, a, m)
        assert a[sr.N] == 3 and a[sr.N_RATE] == 1 and a[sr.SUM_RATE] == b[sr.SUM_RATE]
        assert a[sr.PROGRESS] == b[sr.PROGRESS] and m[sr.MEM_VALID] == 1
    # counted bits alone lose nothing
    a, m = acc.copy(), mem.copy()
    sr.score_step(C, x[2, 0], u[2, 0], sr.ST_QP_NOT_CONV | sr.ST_MIN_SPEED | sr.ST_STATE_BOUND | sr.ST_THETA_WRAP, 0,
                  False, a, m)
    assert a[sr.N] == 3 and a[sr.N_LOST] == 0


def test_summary_and_combine():
    rng = np.random.default_rng(8)
    acc = rng.uniform(0.0, 3.0, (11, 16))
    for k in sr.INT_SLOTS:
        acc[:, k] = rng.integers(0, 5, 11)
    acc[:, sr.SPARE] = 0.0
    acc[3] = 0.0; acc[7] = 0.0                         # kites that were never scored: no max, no min
    acc[7, sr.N_LOST] = 4.0; acc[7, sr.EVER_LOST] = 1.0
    acc[acc[:, sr.N] == 0] *= np.where(np.arange(16) == sr.MIN_SPEED, 0.0, 1.0)
    s = sr.summary(acc)
    scored = acc[:, sr.N] > 0
    assert s[sr.KITES] == 11 and s[sr.N] == acc[:, sr.N].sum() and s[sr.N_LOST] == acc[:, sr.N_LOST].sum()
    assert s[sr.MAX_D] == acc[scored, sr.MAX_D].max() and s[sr.MIN_SPEED] == acc[scored, sr.MIN_SPEED].min()
    assert s[sr.MIN_SPEED] > 0
    np.testing.assert_allclose(s[sr.SUM_D2], acc[:, sr.SUM_D2].sum(), rtol=1e-15)
    # shards combine by +, max, min; a shard without a scored period has neither
    parts = [sr.summary(acc[:3]), sr.summary(acc[3:4]), sr.summary(acc[4:])]
    assert parts[1][sr.N] == 0
    c = ok.score_combine(parts)
    for k in range(16):
        if k in (sr.MAX_D, sr.MIN_SPEED) or k in sr.INT_SLOTS or k == sr.KITES:
            assert c[k] == s[k], k
        else:
            assert abs(c[k] - s[k]) <= 4 * np.finfo(float).eps * s[k], k
    assert ok.score_combine([np.zeros(16)])[sr.MIN_SPEED] == 0.0
    with pytest.raises(ValueError):
        ok.score_combine([])
    d = ok.score_derive(s, dt=0.05)
    assert d["n"] == s[sr.N] and d["kites"] == 11
    assert d["rms_d"] == math.sqrt(s[sr.SUM_D2] / s[sr.N]) and d["mean_u"] == s[sr.SUM_U] / s[sr.N]
    assert d["lost_fraction"] == s[sr.N_LOST] / (s[sr.N] + s[sr.N_LOST])
    assert d["laps"] == s[sr.PROGRESS] / (2 * math.pi) and d["lap_rate"] == d["laps"] / (s[sr.N_RATE] * 0.05)
    assert math.isnan(ok.score_derive(np.zeros(16))["rms_d"])


def test_gpu_test_inputs_meet_the_condition():
    n = 0
    for name, C, pos in sr.gpu_test_positions({k: sr.consts(cfg_of(k)) for k in ("circle", "fourier")}):
        for i, r in enumerate(pos):
            assert sr.condition_ok(C, r), (name, i)
            n += 1
    assert n > 100


def test_rounding_envelope():
    """Worst |float64 - 50-digit| per quantity over the GPU tests' inputs."""
    worst = {k: 0.0 for k in sr.ENVELOPE}
    count = 0
    Cs = {k: sr.consts(cfg_of(k)) for k in ("circle", "fourier")}
    for C, x, u, mem, first in sr.gpu_test_periods(Cs):
        a = sr.period(C, x, u, mem, first)
        b = sr.period(C, x, u, mem, first, mp=True)
        for k in worst:
            if a[k] is not None:
                worst[k] = max(worst[k], float(abs(b[k] - a[k])))
        count += 1
    print(f"rounding envelope over {count} periods (worst |fp64 - 50 digits|), recorded, GPU bar = 32 x recorded:")
    for k, v in worst.items():
        print(f"  {k:7s} measured {v:.3e}   recorded {sr.ENVELOPE[k]:.1e}   bar {sr.bar(k):.2e}")
    for k, v in worst.items():
        assert v <= sr.ENVELOPE[k] <= 1.25 * v, (k, v, sr.ENVELOPE[k])
