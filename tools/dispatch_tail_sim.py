"""Dispatch tail of k_qp_tiled, simulated on the CPU (tools only, no GPU).

One QP wave per kite, one wave at a time per SIMD, 1024 SIMDs: a wave's time
is taken as its interior-point iteration count, and the waves go to the SIMD
that frees first in dispatch order (list scheduling).  Printed per dispatch
key: the makespan over the mean load per SIMD, averaged over the steps, 1.0
being a step without a tail.

Iteration counts come from the oracle on the benchmark's loop (synthetic
fleet, closed loop on the plan's own prediction, episodes as bench.py), or
from the file tools/iter_dist.py writes (--iters FILE.npz, array `iters` of
steps x kites).
  python tools/dispatch_tail_sim.py [--kites 4096] [--steps 33] [--skip 3] [--iters FILE.npz]

--split K adds the two-launch strategies (the two-phase solve): a
first launch that stops every kite at iteration K, a second that resumes the
kites still running, ordered by the previous count or by the residual at K
(its exact value, its decade, its binary exponent).  On every third step the
oracle is probed per kite for that residual (prologue + build_qp + qp_solve
with the cap K); only those steps are scored.  --resume R charges R
iterations per resumed kite (the init phase run again).
  python tools/dispatch_tail_sim.py --split 9 --steps 19 [--resume 0.25]
"""
import argparse
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIMDS = 1024


def oracle_counts(B, steps, episode, N=20, M=2, K=16, probe_k=0):
    from oracle import ffi
    kp = ffi.load_params()
    cfgv = ffi.cfg_vector(dict(ffi.node_config(N=N), qp_form=0))
    xs = ffi.synthetic_states(B)
    x0 = np.zeros((B, 15))
    x0[:, :13] = xs
    for b in range(B):
        x0[b, 13] = ffi.closest_point(cfgv, xs[b, 6:9])
    X = np.zeros((B, N + 1, 15)); U = np.zeros((B, N, 4))
    out, x, probes = [], x0.copy(), {}
    for s in range(steps):
        cold = s % episode == 0
        if cold:
            x = x0.copy()
        if probe_k and s >= 3 and s % 3 == 0:          # the residual at the cap probe_k, per kite
            r = np.zeros(B)
            for b in range(B):
                _, Xb, Ub, _ = ffi.prologue(kp, cfgv, N, M, x[b], X[b], U[b], warm=int(not cold))
                q = ffi.build_qp(kp, cfgv, N, M, Xb, Ub)
                r[b] = ffi.qp_solve(q["H"], q["h"], q["lb"], q["ub"], q["C"], q["c"], probe_k)[1]
            probes[s] = r
        it = np.zeros(B, dtype=np.int32)
        ffi.rti_step(kp, cfgv, N, M, K, x, X, U, warm=int(not cold), iters=it)
        out.append(it.copy())
        x = X[:, 1, :].copy()
    return (np.array(out), probes) if probe_k else np.array(out)


def two_launch(t, k, first_order, key, resume):
    """Makespan over mean load of a launch capped at k plus a launch of the rest
    (larger key first), against the one-launch load t.sum() / SIMDS."""
    t1 = np.minimum(t, k)
    rest = np.nonzero(t > k)[0]
    t2 = t[rest] - k + resume
    load = t.sum() / SIMDS
    m1 = makespan(t1, first_order) * t1.sum() / SIMDS
    m2 = makespan(t2, np.argsort(-key[rest], kind="stable")) * t2.sum() / SIMDS if rest.size else 0.0
    return (m1 + m2) / load


def makespan(t, order):
    free = [0.0] * SIMDS
    heapq.heapify(free)
    end = 0.0
    for i in order:
        e = heapq.heappop(free) + t[i]
        end = max(end, e)
        heapq.heappush(free, e)
    return end / max(t.sum() / SIMDS, 1e-300)


def keys(its, s):
    """Dispatch keys known before step s (larger first)."""
    p1 = its[s - 1].astype(float)
    p2 = its[s - 2].astype(float) if s >= 2 else p1
    p3 = its[s - 3].astype(float) if s >= 3 else p2
    return {
        "unsorted": None,
        "previous count (the present order)": p1,
        "max of the last two": np.maximum(p1, p2),
        "max of the last three": np.maximum(p1, np.maximum(p2, p3)),
        "trend (2 p1 - p2)": 2 * p1 - p2,
        "rise (p1 + max(p1 - p2, 0))": p1 + np.maximum(p1 - p2, 0),
        "fall (p1 + max(p2 - p1, 0))": p1 + np.maximum(p2 - p1, 0),
        "range of the last three": p1 + np.maximum(p1, np.maximum(p2, p3)) - np.minimum(p1, np.minimum(p2, p3)),
        "perfect knowledge of the counts": its[s].astype(float),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kites", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=33)
    ap.add_argument("--skip", type=int, default=3, help="steps before the first scored one (bench.py's warm-up)")
    ap.add_argument("--episode", type=int, default=40)
    ap.add_argument("--iters", default=None)
    ap.add_argument("--split", type=int, default=0, metavar="K", help="two launches split at iteration K (oracle probe)")
    ap.add_argument("--resume", type=float, default=0.0, help="iterations charged per resumed kite")
    a = ap.parse_args()
    if a.split:
        its, probes = oracle_counts(a.kites, a.steps, a.episode, probe_k=a.split)
        res = {}
        for s, r in probes.items():
            t = its[s].astype(float)
            prev = np.argsort(-its[s - 1].astype(float), kind="stable")
            lr = np.log10(np.maximum(r, 1e-300))
            res.setdefault("present (previous count, one launch)", []).append(makespan(t, prev))
            for name, key in (("second sorted by previous count", its[s - 1].astype(float)),
                              ("second sorted by log10(residual)", lr),
                              ("second sorted by its decade", np.floor(lr)),
                              ("second sorted by its binary exponent", np.floor(np.log2(np.maximum(r, 1e-300))))):
                res.setdefault(f"split at {a.split}, {name}", []).append(two_launch(t, a.split, prev, key, a.resume))
            res.setdefault("perfect knowledge, one launch", []).append(makespan(t, np.argsort(-t, kind="stable")))
        print(f"{its.shape[1]} kites, steps {sorted(probes)}, {SIMDS} SIMDs, resume cost {a.resume} iteration")
        for name, v in res.items():
            print(f"  {name:52s} makespan / mean load {np.mean(v):.3f}")
        return
    its = np.load(a.iters)["iters"] if a.iters else oracle_counts(a.kites, a.steps, a.episode)
    res = {}
    for s in range(max(a.skip, 1), its.shape[0]):
        t = its[s].astype(float)
        for name, k in keys(its, s).items():
            order = np.arange(t.size) if k is None else np.argsort(-k, kind="stable")
            res.setdefault(name, []).append(makespan(t, order))
    print(f"{its.shape[1]} kites, steps {max(a.skip, 1)}..{its.shape[0] - 1}, {SIMDS} SIMDs, "
          f"mean iterations {its[max(a.skip, 1):].mean():.3f}")
    for name, v in res.items():
        print(f"  {name:38s} makespan / mean load {np.mean(v):.3f}")


if __name__ == "__main__":
    main()
