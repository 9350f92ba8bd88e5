#!/usr/bin/env python3
"""Generate tests/golden/kite_wind_golden.json (run here, never on the GPU box).

The wind extension of the kite model, restated symbolically in the style of
gen_golden.py (literal w-first quaternion products, the ODE of
kite.cpp:197-317) and evaluated with mpmath at 50 significant digits: a
constant world-frame wind W makes the aerodynamics -- airspeed, angles,
dynamic pressure, the rate-damping terms -- see the air-relative body velocity

    v_a = v - q^-1 (x) [0, W] (x) q

while gravity, the Coriolis term w x v, the tether and the kinematics keep the
inertial v.  It pins, at a few (state, control, wind) triples,

  * f(x, u, W)
  * the exact Jacobians d f / d x (13 x 13) and d f / d W (13 x 3)  (sympy.diff)

The states and controls are rhs cases of kite_golden.json; the winds are up to
1.5 m/s per component, and one triple has zero wind (there f and d f / d x are
gen_golden.py's).

Usage:  python tests/golden/gen_wind_golden.py   (writes kite_wind_golden.json)
"""
from __future__ import annotations

import json
import os

import mpmath as mp
import sympy as sp

from gen_golden import HERE, REPO, load_yaml, mpl, qinv, qmul, to_mp

mp.mp.dps = 50


def kite_wind_symbolic(prm):
    """Returns (x13, u3, W3, f13): kite.cpp:197-317 with the wind in the
    aerodynamic terms only."""
    g = sp.Rational("9.80665")
    ro = sp.Rational("1.2985")
    P = {k: sp.Rational(repr(float(v))) for sec in ("geometry", "inertia", "aerodynamic", "tether")
         for k, v in prm[sec].items()}
    b, c, AR, S = P["b"], P["c"], P["AR"], P["S"]
    Mass, Ixx, Iyy, Izz, Ixz = P["mass"], P["Ixx"], P["Iyy"], P["Izz"], P["Ixz"]
    x = sp.symbols("x0:13", real=True)
    u = sp.symbols("u0:3", real=True)
    W = sp.symbols("W0:3", real=True)
    v = sp.Matrix(x[0:3]); w = sp.Matrix(x[3:6]); r = sp.Matrix(x[6:9]); q = list(x[9:13])
    T, dE, dR = u
    # air-relative body velocity: the wind rotated into the body frame
    Wb = qmul(qmul(qinv(q), [0, W[0], W[1], W[2]]), q)
    va = v - sp.Matrix(Wb[1:4])
    V2 = va.dot(va)
    V = sp.sqrt(V2)
    ss = sp.asin(va[1] / (V + sp.Rational(1, 10000)))
    aoa = sp.atan2(va[2], va[0] + sp.Rational(1, 10000))
    dyn = sp.Rational(1, 2) * ro * V2
    CD = P["CD0_total"] + (P["CL0"] + P["CLa_total"] * aoa) ** 2 / (sp.pi * P["e_oswald"] * AR)
    LIFT = (P["CL0"] + P["CLa_total"] * aoa) * dyn * S + (sp.Rational(1, 4) * P["CLq"] * c * S * ro) * V * w[1]
    DRAG = CD * dyn * S
    SF = (P["CYb"] * ss + P["CYdr"] * dR) * dyn * S \
        + sp.Rational(1, 4) * (P["CYr"] * w[2] + P["CYp"] * w[0]) * (b * ro * S) * V
    q_aoa = [sp.cos(aoa / 2), 0, sp.sin(aoa / 2), 0]
    q_ss = [sp.cos(-ss / 2), 0, 0, sp.sin(-ss / 2)]
    qwb = qmul(q_aoa, q_ss)
    F = qmul(qmul(qinv(qwb), [0, -DRAG, 0, -LIFT]), qwb)
    Fa = sp.Matrix(F[1:4])
    Zde = (-P["CLde"]) * dE * dyn * S
    FE = qmul(qmul(qinv(q_aoa), [0, 0, 0, Zde]), q_aoa)
    Fa = Fa + sp.Matrix(FE[1:4]) + sp.Matrix([0, SF, 0])
    G = qmul(qmul(qinv(q), [0, 0, 0, g]), q)
    Gb = sp.Matrix(G[1:4])
    # tether and kinematics: the inertial velocity
    d_ = sp.sqrt(r.dot(r))
    Rv = d_ - P["length"]
    Rs = -Rv * (r / d_)
    VI = qmul(qmul(q, [0, v[0], v[1], v[2]]), qinv(q))
    vi = sp.Matrix(VI[1:4])
    Rd = (-r / d_) * r.dot(vi) / d_
    hv = 1 / (1 + sp.exp(-4 * (d_ - P["length"])))
    R = (P["Ks"] * Rs + P["Kd"] * Rd) * hv
    RB = qmul(qmul(qinv(q), [0, R[0], R[1], R[2]]), q)
    Rb = sp.Matrix(RB[1:4])
    vdot = (Fa + sp.Matrix([T, 0, 0]) + Rb) / Mass + Gb - w.cross(v)
    L = (P["Cl0"] + P["Clb"] * ss + P["Cldr"] * dR) * dyn * S * b \
        + (P["Clr"] * w[2] + P["Clp"] * w[0]) * (sp.Rational(1, 4) * ro * b ** 2 * S) * V
    M = (P["Cm0"] + P["Cma"] * aoa + P["Cmde"] * dE) * dyn * S * c \
        + P["Cmq"] * (sp.Rational(1, 4) * S * c ** 2 * ro) * w[1] * V
    N = (P["Cn0"] + P["Cnb"] * ss + P["Cndr"] * dR) * dyn * S * b \
        + (P["Cnp"] * w[0] + P["Cnr"] * w[2]) * (sp.Rational(1, 4) * S * b ** 2 * ro) * V
    J = sp.Matrix([[Ixx, 0, Ixz], [0, Iyy, 0], [Ixz, 0, Izz]])
    TR = qmul(qmul(qinv(q_aoa), [0, L, M, N]), q_aoa)
    Ma = sp.Matrix(TR[1:4])
    arm = sp.Matrix([P.get("rx", 0), P.get("ry", 0), P.get("rz", 0)])
    Mt = arm.cross(Rb)
    wdot = J.inv() * (Ma + Mt - w.cross(J * w))
    rdot = vi
    qw = qmul(q, [0, w[0], w[1], w[2]])
    qq = sum(qi * qi for qi in q)
    qdot = [sp.Rational(1, 2) * qw[i] + sp.Rational(1, 2) * (-5) * q[i] * (qq - 1) for i in range(4)]
    f = list(vdot) + list(wdot) + list(rdot) + qdot
    return x, u, W, f


# (index of the rhs case of kite_golden.json, wind in m/s)
TRIPLES = [
    (1, [0.0, 0.0, 0.0]),
    (4, [0.5, -0.3, 0.2]),
    (5, [1.5, 0.0, 0.0]),
    (6, [-0.7, 1.1, -0.4]),
    (7, [0.3, 0.8, 1.5]),
    (8, [-1.5, -1.5, 0.9]),
]


def main():
    x, u, W, f = kite_wind_symbolic(load_yaml(os.path.join(REPO, "data", "umx_radian.yaml")))
    xs = list(x) + list(u) + list(W)
    fn = sp.lambdify(xs, f, modules="mpmath")
    Jx = sp.lambdify(xs, sp.Matrix(f).jacobian(sp.Matrix(list(x))), modules="mpmath")
    Jw = sp.lambdify(xs, sp.Matrix(f).jacobian(sp.Matrix(list(W))), modules="mpmath")
    base = json.load(open(os.path.join(HERE, "kite_golden.json")))["rhs"]
    cases = []
    for idx, wind in TRIPLES:
        c = base[idx]
        args = to_mp(c["x"]) + to_mp(c["u"]) + to_mp(wind)
        fv = [mp.mpf(t) for t in fn(*args)]
        jx = Jx(*args)
        jw = Jw(*args)
        cases.append(dict(source=c["source"], x=c["x"], u=c["u"], wind=wind, f=mpl(fv),
                          Jx=[mpl([jx[i, j] for j in range(13)]) for i in range(13)],
                          Jw=[mpl([jw[i, j] for j in range(3)]) for i in range(13)]))
    out = dict(generator="tests/golden/gen_wind_golden.py (sympy %s, mpmath %s, %d digits)"
               % (sp.__version__, mp.__version__, mp.mp.dps),
               params_file="data/umx_radian.yaml", cases=cases)
    with open(os.path.join(HERE, "kite_wind_golden.json"), "w") as fobj:
        json.dump(out, fobj, indent=1)
    print("wrote kite_wind_golden.json,", len(cases), "cases")


if __name__ == "__main__":
    main()
