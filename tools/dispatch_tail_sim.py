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
"""
import argparse
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIMDS = 1024


def oracle_counts(B, steps, episode, N=20, M=2, K=16):
    from oracle import ffi
    kp = ffi.load_params()
    cfgv = ffi.cfg_vector(dict(ffi.node_config(N=N), qp_form=0))
    xs = ffi.synthetic_states(B)
    x0 = np.zeros((B, 15))
    x0[:, :13] = xs
    for b in range(B):
        x0[b, 13] = ffi.closest_point(cfgv, xs[b, 6:9])
    X = np.zeros((B, N + 1, 15)); U = np.zeros((B, N, 4))
    out, x = [], x0.copy()
    for s in range(steps):
        cold = s % episode == 0
        if cold:
            x = x0.copy()
        it = np.zeros(B, dtype=np.int32)
        ffi.rti_step(kp, cfgv, N, M, K, x, X, U, warm=int(not cold), iters=it)
        out.append(it.copy())
        x = X[:, 1, :].copy()
    return np.array(out)


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
    a = ap.parse_args()
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
