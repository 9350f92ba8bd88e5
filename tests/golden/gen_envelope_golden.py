#!/usr/bin/env python3
"""Generate tests/golden/kite_envelope_golden.json (run on the CPU, never on
the GPU box; needs the built oracle for the path axis of the orbit states).

The same 50-digit sympy / mpmath restatement of the kite model as
gen_golden.py (kite_symbolic, the exact Jacobian, RK4 with the chain rule
through its stages), evaluated at the flight-envelope states of
tests/envelope_states.py instead of the cloud around the base state:

  * rhs: f(x,u) and d f / d [x,u] at every case
  * rk4: one interval tf = 0.05, M = 2 with exact xnext, A, B at the cases
    marked for it, each with S_err_prec24: the error of A, B evaluated with
    mpmath at 24-bit working precision (inputs rounded to 24 bits) against
    the 50-digit values, relative to max(1, |ref|) over A and B -- the
    precision floor of an fp32 sensitivity at that state.

Usage:  python tests/golden/gen_envelope_golden.py
"""
from __future__ import annotations

import json
import os
import sys

import mpmath as mp
import sympy as sp

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_golden import load_model, mpl, to_mp  # noqa: E402
from tests.envelope_states import envelope_cases  # noqa: E402

TF, M_INT = "0.05", 2
THETA = [0.3, -0.4]      # theta, thetadot and the virtual control of the RK4 cases (as gen_golden.py)
UV = [0.7]


def rel(a, ref):
    a = [v for row in a for v in row]
    ref = [v for row in ref for v in row]
    return max(abs(p - q) for p, q in zip(a, ref)) / max(1.0, max(abs(q) for q in ref))


def main():
    model = load_model()
    rhs_cases, rk4_cases = [], []
    for src, xv, uv, want_rk4 in envelope_cases():
        xm, um = to_mp(xv), to_mp(uv)
        fv = model.f_mp(xm, um)
        J = model.jac_mp(xm, um)
        rhs_cases.append(dict(source=src, x=xv, u=uv, f=mpl(fv), J=[mpl(row) for row in J]))
        if not want_rk4:
            continue
        x15, u4 = list(xv) + THETA, list(uv) + UV
        xo, S = model.rk4_sens(to_mp(x15), to_mp(u4), mp.mpf(TF) / M_INT, M_INT)
        A, B = [mpl(r[:15]) for r in S], [mpl(r[15:]) for r in S]
        with mp.workprec(24):
            _, S24 = model.rk4_sens(to_mp(x15), to_mp(u4), mp.mpf(TF) / M_INT, M_INT)
        A24, B24 = [mpl(r[:15]) for r in S24], [mpl(r[15:]) for r in S24]
        rk4_cases.append(dict(source=src, x=x15, u=u4, tf=float(TF), M=M_INT, xnext=mpl(xo), A=A, B=B,
                              S_err_prec24=max(rel(A24, A), rel(B24, B))))
    out = dict(
        generator="tests/golden/gen_envelope_golden.py (sympy %s, mpmath %s, %d digits)"
                  % (sp.__version__, mp.__version__, mp.mp.dps),
        params_file="data/umx_radian.yaml", states="tests/envelope_states.py", rhs=rhs_cases, rk4=rk4_cases,
    )
    path = os.path.join(HERE, "kite_envelope_golden.json")
    text = json.dumps(out, separators=(",", ":")).replace('{"source"', '\n{"source"')
    with open(path, "w") as fobj:
        fobj.write(text + "\n")
    print("wrote", path, "rhs", len(rhs_cases), "rk4", len(rk4_cases), "bytes", len(text) + 1)


if __name__ == "__main__":
    main()
