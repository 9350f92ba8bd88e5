"""State generators of the flight-envelope tests (tests/test_envelope.py) and
of their 50-digit fixture (tests/golden/gen_envelope_golden.py).

Every other GPU parity test draws its kites from ffi.synthetic_states: one
small cloud around ffi.BASE_STATE.  The generators here start from the same
base state and leave that corner: around the path circle (every heading,
gravity direction and theta), through the atan2 quadrants of the angle of
attack, to large sideslip, slack and hard-taut tether, |q| != 1 and the
corners of the control box.  Each regime changes only what it names.
"""
import itertools
import math

import numpy as np

from oracle import ffi

LT = 2.81                                   # tether length, data/umx_radian.yaml
BASE_U = [0.125, 0.0, 0.0]                  # thrust, elevator, rudder of the base cases
ATTITUDE_SEED = 20261019


def qmul(a, b):
    """Hamilton product, w first."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.array([a[0] * b[0] - a[1:] @ b[1:], *(np.cross(a[1:], b[1:]) + a[0] * b[1:] + b[0] * a[1:])])


def qrot(q, v):
    """q (x) [0, v] (x) q^-1 for a unit q."""
    qc = np.array([q[0], -q[1], -q[2], -q[3]])
    return qmul(qmul(q, np.r_[0.0, v]), qc)[1:]


def path_axis(cfgv=None):
    """Unit normal of the node's path circle: normalise(P(0) x P(pi / 2))."""
    cv = ffi.cfg_vector(ffi.node_config()) if cfgv is None else cfgv
    n = np.cross(ffi.path(cv, 0.0)[0], ffi.path(cv, math.pi / 2)[0])
    return n / np.linalg.norm(n)


def rotate_about_path(x13, phi, n):
    """The kite state turned by phi about the path axis n: position r' = q_n r
    q_n^-1, attitude q' = q_n (x) q; body velocities and rates unchanged."""
    qn = np.r_[math.cos(phi / 2), math.sin(phi / 2) * np.asarray(n)]
    x = np.array(x13, dtype=float)
    x[6:9] = qrot(qn, x[6:9])
    x[9:13] = qmul(qn, x[9:13])
    return x


def envelope_cases():
    """[(source, x13, u3, rk4)] of the fixture: source starts with the regime
    name, rk4 marks the cases that also get an RK4 interval."""
    base = ffi.BASE_STATE
    cfg = ffi.node_config()
    n = path_axis()
    out = []

    def add(src, x, u=BASE_U, rk4=False):
        out.append((src, [float(t) for t in x], [float(t) for t in u], rk4))

    for k in range(8):
        add(f"orbit k={k} phi={45 * k}deg", rotate_about_path(base, math.radians(45.0 * k), n), rk4=k in (2, 4, 6))
    rng = np.random.default_rng(ATTITUDE_SEED)
    for i in range(4):
        q = rng.normal(size=4)
        x = base.copy(); x[9:13] = q / np.linalg.norm(q)
        add(f"attitude [{i}] seed={ATTITUDE_SEED}", x, rk4=i == 0)
    for v, rk in (((2.1, 0.0, 0.1), True), ((8.0, 0.3, 0.8), False), ((15.0, 0.5, 1.0), True)):
        x = base.copy(); x[0:3] = v
        add(f"airspeed v={v}", x, rk4=rk)
    for v, rk in (((0.7, 0.2, 4.0), True), ((0.7, 0.2, -4.0), False), ((-3.0, 0.4, 1.0), True), ((-3.0, 0.4, -1.0), False)):
        x = base.copy(); x[0:3] = v
        add(f"aoa v={v}", x, rk4=rk)
    for v, rk in (((3.0, 1.7, 0.5), True), ((3.0, -1.7, 0.5), False), ((1.2, 4.0, 0.5), False), ((1.2, -4.0, 0.5), True)):
        x = base.copy(); x[0:3] = v
        add(f"sideslip v={v}", x, rk4=rk)
    for d in (-1.5, -0.05, 0.05, 1.0):
        for sign in (1.0, -1.0):
            x = base.copy()
            x[6:9] *= (LT + d) / np.linalg.norm(base[6:9])
            x[0:3] *= sign
            add(f"tether |r|=Lt{d:+g} v={'base' if sign > 0 else 'negated'}", x,
                rk4=(d, sign) in ((-1.5, 1.0), (1.0, -1.0)))
    for s in (0.8, 1.2):
        x = base.copy(); x[9:13] *= s
        add(f"qnorm |q|={s}", x, rk4=True)
    for i, u in enumerate(itertools.product(*zip(cfg["lbu"][:3], cfg["ubu"][:3]))):
        add(f"controls corner {i}", base, u, rk4=i == 5)
    return out


def regime(source):
    return source.split()[0]


def orbit_batch(B, N=20, offset=0):
    """(B, 15) RTI inputs around the orbit: kite b is synthetic_states(offset)[b]
    turned by (b mod 8) 45 deg about the path axis, theta the closest point of
    the path, thetadot 0."""
    cv = ffi.cfg_vector(ffi.node_config(N=N))
    n = path_axis(cv)
    xs = ffi.synthetic_states(B, offset=offset)
    x0 = np.zeros((B, 15))
    for b in range(B):
        x0[b, :13] = rotate_about_path(xs[b], math.radians(45.0 * (b % 8)), n)
        x0[b, 13] = ffi.closest_point(cv, x0[b, 6:9])
    return x0


def wrapped(x0, kites=range(8, 16)):
    """x0 with 2 pi added to the input theta of the given kites, signed by
    theta's own sign (the prologue wraps it back, status bit 16)."""
    x = x0.copy()
    for b in kites:
        x[b, 13] += math.copysign(2 * math.pi, x[b, 13])
    return x
