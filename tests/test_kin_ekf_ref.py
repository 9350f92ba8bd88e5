"""CPU tests of the kinematic EKF's numpy reference (tests/kin_ekf_ref.py), the
filter tests/test_kin_ekf.py compares the HIP kernel against: its Jacobian
against a complex-step derivative, its model against the pinned oracle's
kinematic rows, the pose frame, the two-pose initialisation, and the open-loop
convergence the GPU filter has to repeat."""
import numpy as np

import openkite_amd as ok
from oracle import ffi
from tests import kin_ekf_ref as ref

RHS_TOL = 1e-13     # tests/test_oracle.py: relative, f
JAC_TOL = 1e-12     # tests/test_oracle.py: relative, df/dx


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def seeded_states(n, seed=5):
    """n states around the flight envelope; the quaternion norm runs over 0.9 .. 1.1."""
    rng = np.random.default_rng(seed)
    x = ffi.synthetic_states(n, offset=800)
    x[:, :6] += rng.normal(size=(n, 6)) * 0.5
    q = x[:, 9:13] + rng.normal(size=(n, 4)) * 0.3
    x[:, 9:13] = q / np.linalg.norm(q, axis=1, keepdims=True) * np.linspace(0.9, 1.1, n)[:, None]
    return x


def test_analytic_jacobian_vs_complex_step():
    """f is a polynomial, so the complex step is exact to rounding: 1e-14 of the largest entry."""
    worst = 0.0
    for x in seeded_states(32):
        J = ref.jac(x)
        Jc = np.zeros((13, 13))
        for k in range(13):
            xc = x.astype(complex)
            xc[k] += 1e-30j
            Jc[:, k] = ref.f(xc).imag / 1e-30
        e = np.abs(J - Jc).max() / np.abs(Jc).max()
        worst = max(worst, e)
        assert e < 1e-14, e
        assert not J[:6].any()                                  # v_b and w_b are random walks
        assert np.count_nonzero(J) <= 49
    print(f"analytic J vs complex step, worst of 32 states: {worst:.2e} of the largest entry")


def test_kinematic_rows_are_the_pinned_oracles(kp):
    """At unit q the kinematics of the kite model and of the filter's model are
    the same functions (r' with conj(q); q' differs only in the stabiliser's
    lambda, whose value vanishes at q.q = 1): rows 6..12 of f within the golden
    bar of f.  The stabiliser's derivative does not vanish, so of J only rows
    6..8 (r') are shared, within the golden bar of df."""
    xs = ffi.synthetic_states(8, offset=800)
    for x in xs:
        x = x.copy()
        x[9:13] /= np.linalg.norm(x[9:13])
        u = np.array([0.12, 0.03, -0.02])
        fo = ffi.rhs(kp, x, u)
        assert rel(ref.f(x)[6:], fo[6:]) < RHS_TOL
        Jo = ffi.rhs_jac(kp, x, u)[:, :13]
        assert rel(ref.jac(x)[6:9], Jo[6:9]) < JAC_TOL
        # and the q rows differ by the two stabilisers' derivatives: (lambda_kin - lambda_kite) q q'
        q = x[9:13]
        assert rel(ref.jac(x)[9:, 9:] - Jo[9:, 9:13], (ref.LAMBDA + 5.0) * np.outer(q, q)) < JAC_TOL


def test_pose_frame():
    d = ok.pose_frame_default().to_dict()
    assert d == dict(offset=(-0.09, 0.0, -0.02), rotation=(0.0, -1.0, 0.0, 0.0), shift=(0.0, 0.0, 2.77))
    assert d == {k: tuple(v) for k, v in ref.DEFAULT_FRAME.items()}
    rng = np.random.default_rng(2)
    z = np.r_[rng.normal(size=3), rng.normal(size=4)]
    np.testing.assert_allclose(ref.frame(z, ref.IDENTITY_FRAME), z, rtol=1e-15, atol=0.0)
    np.testing.assert_array_equal(ref.frame(z, None), z)
    # by hand: attitude j (half a turn about y) turns the offset into (0.09, 0, 0.02);
    # the frame's rotation -i is half a turn about x, (x, y, z) -> (x, -y, -z), and
    # (-i) j (i) = -j; then the shift
    got = ref.frame([1.0, 2.0, 3.0, 0.0, 0.0, 1.0, 0.0], ref.DEFAULT_FRAME)
    np.testing.assert_allclose(got, [1.09, -2.0, -3.02 + 2.77, 0.0, 0.0, -1.0, 0.0], rtol=0.0, atol=2e-15)


def _pose_pair(x, dt):
    """The pose now and dt later under the model's own RK4 (16 steps)."""
    y = x.copy()
    for _ in range(16):
        y = ref.rk4(y, dt / 16)
    return x[6:13].copy(), y[6:13].copy()


def test_two_pose_initialisation_is_first_order():
    """The finite differences recover (v_b, w_b) to first order in dt: halving
    dt halves the error (ratio 2 +- 0.2).  The first-order term is the
    velocity's, dt/2 w x v (the mean of the rotating velocity against its
    start); for constant rates w_b's own error is of second order, so the ratio
    is asserted on the error of (v_b, w_b) together and on v_b's."""
    xs = ffi.synthetic_states(4, offset=800)
    for x in xs:
        x = x.copy()
        x[9:13] /= np.linalg.norm(x[9:13])
        err = []
        for dt in (0.02, 0.01):
            mp, mn = _pose_pair(x, dt)
            x13, st = ref.init(mp, mn, dt)
            assert st == 0
            np.testing.assert_array_equal(x13[6:], mn)
            err.append(x13[:6] - x[:6])
            flipped, _ = ref.init(mp, np.r_[mn[:3], -mn[3:]], dt)
            np.testing.assert_array_equal(flipped[:6], x13[:6])          # bitwise
            np.testing.assert_array_equal(flipped[9:], -mn[3:])           # the state keeps the measured sign
        ratio = np.linalg.norm(err[0]) / np.linalg.norm(err[1])
        ratio_v = np.linalg.norm(err[0][:3]) / np.linalg.norm(err[1][:3])
        print(f"init error at dt 0.02 / 0.01: {np.linalg.norm(err[0]):.3e} / {np.linalg.norm(err[1]):.3e}, "
              f"ratio {ratio:.3f} (v_b alone {ratio_v:.3f})")
        assert abs(ratio - 2.0) < 0.2
        assert abs(ratio_v - 2.0) < 0.2
    assert ref.init(mp, mn, 0.0) == (None, ref.EKF_INIT_BAD)
    assert ref.init(mp, np.r_[np.nan, mn[1:]], 0.02) == (None, ref.EKF_INIT_BAD)


# ---- the open-loop scenario, shared with tests/test_kin_ekf.py ---------------------
# The scenario first asked for -- truth the oracle's kite model (ffi.rk4, thrust
# 0.12) from ffi.synthetic_states, 25 periods of 0.02 s -- is one the reference
# filter cannot meet the bar in, at any number of periods.  Measured (printed by
# the test below): those states accelerate at |v_b'| = 30 .. 55 m/s^2 (taut
# tether, far from trim), while the filter, whose v_b is a random walk that only
# the position innovations correct, follows a velocity with a time constant of
# about 35 periods under the default covariances; the ratio of the mean |v_b
# error| is 3.3 after 25 periods and stays between 1 and 4 up to 100.  Relaxing
# the tether does not help (the free airframe leaves these states at 30 m/s^2 as
# well).  So the scenario, not the bar, is changed, in the two ways foreseen: the
# truth acceleration is zero (the truth flies the rigid-body kinematics from the
# same seeded states: constant body rates, the motion the filter models) and
# the run is 50 periods (25 reach 0.51, just above the bar).  Measurement noise,
# initial error, dt, substeps, B and the covariances are as asked.
OPEN_LOOP = dict(B=8, periods=50, dt=0.02, substeps=5, sigma0=0.3, seed=11, offset=700)
POSE_SIGMA = np.array([0.01] * 3 + [1e-4, 5e-3, 5e-3, 5e-3])     # sqrt(diag V), kiteEKF.cpp:6-13


def open_loop_data(kp=None, periods=None):
    """(truth (periods + 1, B, 13), z (periods, B, 7), est0 (B, 13)): the seeded
    states flown open loop, the noisy poses, the start.  kp None: the truth is
    the kinematic model; kp given: the oracle's kite model at thrust 0.12."""
    s = OPEN_LOOP
    periods = s["periods"] if periods is None else periods
    rng = np.random.default_rng(s["seed"])
    truth = [ffi.synthetic_states(s["B"], offset=s["offset"])]
    est0 = truth[0].copy()
    est0[:, :6] += rng.normal(size=(s["B"], 6)) * s["sigma0"]
    zs = []
    for _ in range(periods):
        nxt = np.zeros_like(truth[-1])
        for b in range(s["B"]):
            if kp is None:
                nxt[b] = ref.rk4(truth[-1][b], s["dt"])
            else:
                x15 = np.zeros(15); x15[:13] = truth[-1][b]
                nxt[b] = ffi.rk4(kp, x15, np.array([0.12, 0.0, 0.0, 0.0]), s["dt"], 1)[:13]
        truth.append(nxt)
        zs.append(nxt[:, 6:13] + rng.normal(size=(s["B"], 7)) * POSE_SIGMA)
    return np.array(truth), np.array(zs), est0


def _reference_run(truth, zs, est):
    s = OPEN_LOOP
    W, V, P0 = ok.ekf_default_covariances()
    P = np.repeat(P0[None], s["B"], axis=0)
    est = est.copy()
    err0 = np.abs(est - truth[0])[:, :3].mean()
    for k in range(len(zs)):
        for b in range(s["B"]):
            est[b], P[b], st = ref.step(est[b], P[b], s["dt"], s["substeps"], zs[k][b], W, V)
            assert st == 0
    return err0, np.abs(est - truth[-1])[:, :3].mean(), P


def test_open_loop_reference_converges(kp):
    """The reference filter on the scenario above: the mean |v_b error| falls
    below half its initial value (test_kite_ekf_mirror_tracks_plant's bar) with
    the default covariances.  Measured: 0.210 -> 0.052, ratio 0.25.  The run
    against the oracle's kite is printed next to it, not asserted (ratio 3.3)."""
    err0, err1, P = _reference_run(*open_loop_data())
    print(f"open loop, reference filter: mean |v_b error| {err0:.4f} -> {err1:.4f}, ratio {err1 / err0:.3f}")
    k0, k1, _ = _reference_run(*open_loop_data(kp, periods=25))
    acc = [np.linalg.norm(ffi.rhs(kp, x, [0.12, 0.0, 0.0])[:3]) for x in ffi.synthetic_states(8, offset=700)]
    print(f"  against the oracle's kite (|v_b'| {min(acc):.0f} .. {max(acc):.0f} m/s^2), 25 periods: "
          f"{k0:.4f} -> {k1:.4f}, ratio {k1 / k0:.2f}")
    assert np.all(np.isfinite(P))
    assert err1 < 0.5 * err0, (err0, err1)
