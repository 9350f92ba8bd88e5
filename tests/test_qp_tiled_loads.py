"""k_qp_tiled's loads at the batch sizes where their indexing can go wrong
(N = 20, the tiled QP): one kite, a batch that is no multiple of 4 (k_expand20
packs four kites per wave) and one that is no multiple of 64.

After one cold step the condensed QP read back through get_qp (H reassembled
from the tile layout k_condense20 stores and k_qp_tiled loads) is symmetric
and meets the oracle's at the bar of test_gpu_parity.py's condensed-QP test
(1e-11), for every kite; and a kite's plan does not depend on the batch it is
solved in: B = 5 equals the first 5 kites of B = 65 bitwise.
"""
import numpy as np
import pytest

import openkite_amd as ok
from oracle import ffi
from test_gpu_parity import M, N, condensed_cfgv, gpu_to_oracle_perm, x0_batch

pytestmark = pytest.mark.gpu

BATCHES = (1, 5, 65)
QP_TOL = 1e-11      # condensed QP (H, h, C) against the oracle, test_gpu_parity.py


@pytest.fixture(scope="module")
def x0():
    return x0_batch(max(BATCHES))


@pytest.fixture(scope="module")
def oracle_qp(kp, x0):
    """The oracle's condensed QP of every kite's cold step (computed once)."""
    cfgv = condensed_cfgv()
    qs = []
    for b in range(max(BATCHES)):
        _, X, U, _ = ffi.prologue(kp, cfgv, N, M, x0[b], np.zeros((N + 1, 15)), np.zeros((N, 4)), warm=0)
        q = ffi.build_qp(kp, cfgv, N, M, X, U)
        qs.append({k: np.array(q[k]) for k in ("H", "h", "C")})
    return qs


@pytest.fixture(scope="module")
def cold_steps(x0):
    """One cold step per batch size: the plan and every kite's QP."""
    out = {}
    for B in BATCHES:
        g = ok.BatchNMPC(ok.load_properties(), ok.default_config(qp_kernel=2), B)
        try:
            r = g.step(x0[:B])
            out[B] = dict(u0=r["u0"].copy(), traj=r["traj"].copy(), qp=[g.get_qp(b) for b in range(B)])
        finally:
            g.close()
    return out


@pytest.mark.parametrize("B", BATCHES)
def test_tiled_qp_readback_vs_oracle(B, cold_steps, oracle_qp):
    perm = gpu_to_oracle_perm(N)
    for b in range(B):
        gq, q = cold_steps[B]["qp"][b], oracle_qp[b]
        assert np.array_equal(gq["H"], gq["H"].T), (B, b)
        Hg = np.zeros_like(q["H"]); Hg[np.ix_(perm, perm)] = gq["H"]
        hg = np.zeros_like(q["h"]); hg[perm] = gq["h"]
        Cg = np.zeros((N, 4 * N + 2)); Cg[:, perm] = gq["C"]
        eH = np.abs(Hg - q["H"]).max() / np.abs(q["H"]).max()
        eh = np.abs(hg - q["h"]).max() / max(1.0, np.abs(q["h"]).max())
        eC = np.abs(Cg - q["C"]).max() / max(1.0, np.abs(q["C"]).max())
        assert eH < QP_TOL and eh < QP_TOL and eC < QP_TOL, (B, b, eH, eh, eC)


def test_plan_independent_of_batch(cold_steps):
    a, c = cold_steps[5], cold_steps[65]
    for k in ("u0", "traj"):
        assert np.array_equal(a[k].view(np.uint64), c[k][:5].view(np.uint64)), k
