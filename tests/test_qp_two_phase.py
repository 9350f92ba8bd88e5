"""The two-phase tiled QP (kite_nmpc_set_qp_split, N = 20): the main solve
stopped at the top of interior-point iteration `split_iteration`, the kites
still running resumed from a checkpoint in a second launch ordered by their
residual.  No operation changes, so a context that always splits must equal
one that never does bit for bit -- plans, diagnostics, status words, residuals
and iteration counts, compared as integer views so that NaNs compare too.

The loop is the benchmark's: synthetic launch states, one cold step, then warm
steps closed on the plan's own prediction (node 1).

The first test also wants the three ways a kite can meet the split: converged
before it, exactly at it, and past it.  On the first six steps of this loop no
kite of the synthetic fleet stops before iteration 9 (the oracle's counts over
kites 0 .. 51599 there: 9 .. 16); the first that does is kite 2416 at step 12
(8 iterations), then kites 2427 and 2513 at step 18.  So the batch starts at
that kite (SEED_OFFSET) and the loop goes on to step 18: the cold step and the
five warm steps first, compared like every later one.
"""
import numpy as np
import pytest

import openkite_amd as ok
from test_gpu_parity import x0_batch

pytestmark = pytest.mark.gpu

K = 16
WARM_STEPS = 5
SEED_OFFSET = 2416   # first kite of the B = 129 batch (see above)
LONG_WARM_STEPS = 18
W_BOUND = 3.0        # bench.py --rate-bound 3


def _ctx(B, mode, rate_bound=0.0):
    cfg = ok.default_config(N=20, M=2, qp_iters=K, qp_kernel=2)
    if rate_bound > 0.0:
        for i in range(3, 6):
            cfg.lbx[i], cfg.ubx[i] = -rate_bound, rate_bound
    g = ok.BatchNMPC(ok.load_properties(), cfg, B)
    g.set_qp_split(mode)
    return g


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _loop(g, x0, steps):
    """steps closed-loop steps from x0 (the first cold); per step every output."""
    out, x = [], x0.copy()
    for _ in range(steps):
        r = g.step(x)
        kkt, iters = g.qp_stats()
        # diag without its last column: comp_time_ms is the host's wall clock, no
        # output of the solve (the residual it replaces on the host is `kkt`)
        out.append(dict(u0=r["u0"].copy(), traj=r["traj"].copy(), diag=r["diag"][:, :5].copy(),
                        status=np.asarray(r["status"]).copy(), kkt=kkt.copy(), iters=iters.copy()))
        x = r["traj"][:, 1, :].copy()
    return out


def _pair(B, x0, steps, rate_bound=0.0):
    """The same loop on a never-split and an always-split context."""
    res = []
    for mode in (ok.QP_SPLIT_NEVER, 1):
        g = _ctx(B, mode, rate_bound)
        try:
            q0 = g.qp_split()
            o = _loop(g, x0, steps)
            q1 = g.qp_split()
        finally:
            g.close()
        res.append((o, q0, q1))
    return res


def _assert_equal(never, split, kites=None, keys=("u0", "traj", "diag", "status", "kkt", "iters")):
    for s, (a, b) in enumerate(zip(never, split)):
        for k in keys:
            va, vb = (a[k], b[k]) if kites is None else (a[k][kites], b[k][kites])
            assert np.array_equal(_bits(va), _bits(vb)), (s, k)


@pytest.fixture(scope="module")
def pair129():
    return _pair(129, x0_batch(129, offset=SEED_OFFSET), 1 + LONG_WARM_STEPS)


def test_forced_split_equals_never_bitwise(pair129):
    (never, n0, n1), (split, s0, s1) = pair129
    assert not n0["active"] and n1["split_launches"] == 0
    assert s0["active"] and s1["split_launches"] > 0
    _assert_equal(never, split)
    # the three ways a kite can meet the split all occur on this loop
    it = np.concatenate([o["iters"] for o in never])
    ks = s0["split_iteration"]
    print("iteration counts:", np.bincount(it, minlength=K + 1), "split at", ks)
    assert 0 < ks < K
    assert (it < ks).any(), "no kite converged before the split"
    assert (it == ks).any(), "no kite converged exactly at the split"
    assert (it > ks).any(), "no kite ran past the split"


def test_lazy_rows_after_a_split_solve():
    B = 64
    (never, _, _), (split, s0, s1) = _pair(B, x0_batch(B), 1 + WARM_STEPS, rate_bound=W_BOUND)
    assert s0["active"] and s1["split_launches"] > 0
    _assert_equal(never, split)
    # the tight rate box binds on this loop: rows were added and kites solved
    # again by the lazy instance from the split solve's hand-over
    w = np.concatenate([np.abs(o["traj"][:, 1:, 3:6]).reshape(B, -1).max(axis=1) for o in never])
    at_bound = np.isfinite(w) & (w > W_BOUND - 1e-6)
    print("kite-steps at the rate bound:", int(at_bound.sum()), "of", w.size)
    assert at_bound.any()


def test_poisoned_kite():
    B, bad = 64, 37
    x0 = x0_batch(B)
    res = []
    for mode in (ok.QP_SPLIT_NEVER, 1):
        g = _ctx(B, mode)
        try:
            o = _loop(g, x0, 2)
            x = o[-1]["traj"][:, 1, :].copy()
            x[bad, 3] = np.nan                       # a non-finite measured state
            o += _loop(g, x, 2)
        finally:
            g.close()
        res.append(o)
    never, split = res
    others = np.arange(B) != bad
    _assert_equal(never, split, kites=others)
    _assert_equal(never, split, kites=np.array([bad]), keys=("status",))
    assert any(o["status"][bad] != 0 for o in never[2:])


def test_auto_mode_keeps_small_batches_whole():
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(N=20, M=2, qp_iters=K, qp_kernel=2), 64)
    try:
        q = g.qp_split()
        assert q["mode"] == ok.QP_SPLIT_AUTO and not q["active"]
        _loop(g, x0_batch(64), 2)
        assert g.qp_split()["split_launches"] == 0
        g.set_qp_split(1)
        assert g.qp_split()["active"]
        g.set_qp_split(ok.QP_SPLIT_AUTO)
        assert not g.qp_split()["active"]
        with pytest.raises(Exception):
            g.set_qp_split(-2)
    finally:
        g.close()
