"""The five EKF kernels after their measurement update moved into
csrc/ekf_update.hpp: nothing they produce may move.

Every case of run_cases() gives the x, P and status that
tests/golden/ekf_bits_golden.npz records from the commit before the move
(tests/golden/gen_ekf_bits_golden.py), bit for bit.  The bits are tied to the
compiler that built both sides: a ROCm release that contracts or schedules the
fp64 arithmetic differently moves them with no change to the source, and the
fixture is then recorded again from the parent commit under that compiler.

Cases, all at count 5 on a context of B = 5 (one full block of four kites and a
ragged one), from five flight-envelope states (tests/envelope_states.py):
  k_ekf, k_ekf_pk            with and without z
  k_ekf_wind, k_ekf_wind_pk  substeps 1 and 3, with and without z; kite 2
                             non-finite on entry; kite 3 with an innovation
                             covariance that is not positive definite
  k_ekf_kin                  substeps 1 and 3, with and without z, with and
                             without a frame (kite 1's measured quaternion is
                             opposite in sign to the estimate); kite 2
                             non-finite on entry; V = -I
The _pk kernels run under perturb_params rows with KITE_EST_MODEL_CONTROLLER.
"""
import os

import numpy as np
import pytest

import openkite_amd as ok

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ekf_bits_golden.npz")
B = 5
DT = 0.02
SEED = 20261021
SOURCES = ("orbit k=3", "attitude [1]", "aoa v=(0.7, 0.2, 4.0)", "sideslip v=(3.0, -1.7, 0.5)", "controls corner 5")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.astype(np.int32)


def seeded_inputs():
    """The inputs of every case: five envelope states with their controls, a
    generic SPD covariance per filter, measurements 0.01 off the estimate."""
    from tests import envelope_states as es
    from tests import kin_ekf_ref as kref
    from tests.test_kin_ekf import unframe
    cases = es.envelope_cases()
    pick = [next(c for c in cases if c[0].startswith(s)) for s in SOURCES]
    rng = np.random.default_rng(SEED)
    x13 = np.array([c[1] for c in pick])
    u = np.array([c[2] for c in pick])
    x16 = np.concatenate([x13, rng.uniform(-1.5, 1.5, (B, 3))], axis=1)
    W13, V, P13 = ok.ekf_default_covariances()
    W16, _, P16 = ok.wind_ekf_default_covariances()
    P16[13:, 13:] = 0.04 * np.eye(3)
    G = rng.normal(size=(B, 16, 16)) * 0.01
    GG = G @ G.transpose(0, 2, 1)
    P16 = P16[None] + GG
    P13 = P13[None] + GG[:, :13, :13]
    z = x13[:, 6:13] + rng.normal(size=(B, 7)) * 0.01
    zk = z.copy()
    zk[1, 3:] = -zk[1, 3:]                     # q and -q are one attitude
    zf = np.array([unframe(zb, kref.DEFAULT_FRAME) for zb in zk])
    return dict(x13=x13, x16=x16, u=u, P13=P13, P16=P16, z=z, zk=zk, zf=zf, W13=W13, W16=W16, V=V)


def run_cases(inp=None):
    """{name: bits} of every case, through the host entry points."""
    i = seeded_inputs() if inp is None else inp
    out = {}

    def put(name, res):
        for tag, a in zip(("x", "P", "st"), res):
            out[f"{name}/{tag}"] = bits(a)

    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(), B)
    try:
        for kern in ("hom", "pk"):
            if kern == "pk":
                g.set_params(ok.perturb_params(g.params, B, 0.1, seed=1))
                g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
            for up in (False, True):
                put(f"ekf_{kern}/z{int(up)}",
                    g.ekf_step(i["x13"], i["u"], i["P13"], DT, i["z"] if up else None, i["W13"], i["V"]))
                for s in (1, 3):
                    put(f"wind_{kern}/s{s}/z{int(up)}",
                        g.wind_ekf_step(i["x16"], i["u"], i["P16"], DT, s, i["z"] if up else None, i["W16"], i["V"]))
            bad = i["x16"].copy(); bad[2, 4] = np.nan
            put(f"wind_{kern}/nan", g.wind_ekf_step(bad, i["u"], i["P16"], DT, 3, i["z"], i["W16"], i["V"]))
            Pn = i["P16"].copy(); Pn[3, 6:13, 6:13] = -np.eye(7)
            put(f"wind_{kern}/notpd", g.wind_ekf_step(i["x16"], i["u"], Pn, DT, 1, i["z"], i["W16"], i["V"]))
        for framed in (False, True):
            fr = ok.pose_frame_default() if framed else None
            zz = i["zf"] if framed else i["zk"]
            for s in (1, 3):
                for up in (False, True):
                    put(f"kin/s{s}/z{int(up)}/f{int(framed)}",
                        g.kin_ekf_step(i["x13"], i["P13"], DT, s, zz if up else None, i["W13"], i["V"], fr))
        bad = i["x13"].copy(); bad[2, 4] = np.nan
        put("kin/nan", g.kin_ekf_step(bad, i["P13"], DT, 3, i["zk"], i["W13"], i["V"], None))
        put("kin/notpd", g.kin_ekf_step(i["x13"], i["P13"], DT, 3, i["zk"], i["W13"], -np.eye(7), None))
    finally:
        g.close()
    return out


@pytest.mark.gpu
def test_ekf_kernels_bitwise_vs_recorded():
    got = run_cases()
    with np.load(GOLDEN) as want:
        assert sorted(want.files) == sorted(got)
        moved = [k for k in sorted(got) if not np.array_equal(got[k], want[k])]
    assert not moved, moved
    # the recorded runs took the paths they name
    assert got["wind_hom/nan/st"].tolist() == [0, 0, ok.EKF_NAN, 0, 0]
    assert got["wind_pk/notpd/st"].tolist() == [0, 0, 0, ok.EKF_S_NOT_PD, 0]
    assert got["kin/nan/st"].tolist() == [0, 0, ok.EKF_NAN, 0, 0]
    assert got["kin/notpd/st"].tolist() == [ok.EKF_S_NOT_PD] * B
    assert not any(got[k].any() for k in got if k.endswith("/st") and "nan" not in k and "notpd" not in k)
