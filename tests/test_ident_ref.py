"""CPU side of the aerodynamic parameter identification: the reference the GPU
tests compare against (tests/ident_ref.py) is itself checked here, with its
iteration rule, h = 0.02, substeps = 2, states from
``ffi.synthetic_states(offset=3000)``, the 21 perturbed by +-10 %, sinusoidal
thrust, elevator and rudder.

  * F_p by central differences is exact up to rounding (two step sizes agree),
    and the prediction is ``ffi.rk4``;
  * noiseless logs of T = 8, 16, 32, 64 samples with L = 1, 4, T recover the
    truth (measured <= 1e-12 scaled error within 6 evaluations; bar 1e-10);
  * rudder held at exactly 0: CYdr, Cndr, Cldr come back bitwise equal to the
    input, the others are recovered (measured 3e-13; bar 1e-10);
  * truth outside a +-5 % box: monotone cost, final projected gradient
    <= 1e-9 x the initial one (measured 4e-12), result inside the box;
  * noise of 1e-3 on every state, T = 40, L = 1 and 4, box 0.5: projected
    gradient ratio <= 1e-6 after 12 evaluations (measured 5e-13 and 3e-12);
  * round trips of the host-only surface: default config, parameter index,
    save_properties -> load_properties, struct layout.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import openkite_amd as ok
from oracle import ffi
from tests import ident_ref as ref

H, SUB = 0.02, 2
INF = math.inf


def _cfg(**kw):
    base = dict(h=H, substeps=SUB, lb_rel=INF, ub_rel=INF)
    base.update(kw)
    return ok.ident_default_config(**base)


def _truth(kp, seed, rel=0.1):
    """The nominal row with the 21 perturbed by +-rel."""
    return ok.perturb_params(kp, 1, rel, seed, fields=ok.IDENT_FIELDS)[0]


def _scaled_err(row, truth, kp):
    return float(np.abs((row[ref.IDX] - truth[ref.IDX]) / ref.scales(kp)).max())


@pytest.fixture(scope="module")
def x0():
    return ffi.synthetic_states(1, offset=3000)[0]


def test_fp_central_difference_is_exact_and_prediction_is_rk4(kp, x0):
    u = np.array([0.13, 0.05, -0.04])
    F1, F2 = ref.dfdp(kp, x0, u, 0.2), ref.dfdp(kp, x0, u, 0.05)
    rel = np.abs(F1 - F2).max() / np.abs(F1).max()
    print(f"F_p, steps 0.2 vs 0.05: {rel:.2e}")
    assert rel < 1e-11
    assert np.all(F1[6:] == 0.0)                       # the kinematics do not see the 21
    # four chained intervals: S with the two steps, x^ against ffi.rk4
    xa, Sa = x0.copy(), np.zeros((13, 21))
    xb, Sb = x0.copy(), np.zeros((13, 21))
    for _ in range(4):
        xa, Sa = ref.interval(kp, xa, Sa, u, H, SUB, 0.2)
        xb, Sb = ref.interval(kp, xb, Sb, u, H, SUB, 0.05)
    relS = np.abs(Sa - Sb).max() / np.abs(Sa).max()
    x15 = np.zeros(15); x15[:13] = x0
    xr = ffi.rk4(kp, x15, np.r_[u, 0.0], H / SUB, 4 * SUB)[:13]
    relx = np.abs(xa - xr).max() / np.abs(xr).max()
    print(f"S after four intervals: {relS:.2e}, x^ vs ffi.rk4: {relx:.2e}")
    assert relS < 1e-12 and relx < 1e-14


def test_sensitivity_matches_a_parameter_difference(kp, x0):
    """S is the derivative of the prediction: against a central difference of
    ffi.rk4 in each parameter (only to the difference's own 1e-6)."""
    u = np.array([0.13, 0.05, -0.04])
    _, S = ref.sens(kp, x0, u, H, SUB)
    s = ref.scales(kp)
    x15 = np.zeros(15); x15[:13] = x0
    for j in range(21):
        d = 1e-4 * s[j]
        kpp, kpm = kp.copy(), kp.copy()
        kpp[ref.IDX[j]] += d; kpm[ref.IDX[j]] -= d
        fd = (ffi.rk4(kpp, x15, np.r_[u, 0.0], H / SUB, SUB) - ffi.rk4(kpm, x15, np.r_[u, 0.0], H / SUB, SUB))[:13]
        fd /= kpp[ref.IDX[j]] - kpm[ref.IDX[j]]
        assert np.abs(fd - S[:, j]).max() <= 1e-6 * max(1.0, np.abs(S[:, j]).max()), j


@pytest.mark.parametrize("T", [8, 16, 32, 64])
@pytest.mark.parametrize("L", [1, 4, 0])
def test_noiseless_logs_recover_the_truth(kp, x0, T, L):
    L = L or T
    truth = _truth(kp, 11)
    U = ref.controls(T, H, 3)
    X = ref.make_log(truth, x0, U, H, SUB)
    r = ref.identify(kp, X, U, _cfg(segment=L, iters=6))
    err = _scaled_err(r["params"], truth, kp)
    print(f"T={T} L={L}: scaled error {err:.2e}, evals {r['evals']}, cost {r['cost0']:.2e} -> {r['cost']:.2e}")
    assert err <= 1e-10
    assert r["evals"] <= 6 and r["cost"] <= r["cost0"]


def test_unexcited_parameters_stay_bitwise(kp, x0):
    truth = _truth(kp, 12)
    T = 16
    U = ref.controls(T, H, 4, rudder=False)
    X = ref.make_log(truth, x0, U, H, SUB)
    r = ref.identify(kp, X, U, _cfg(iters=6))
    rud = [ok.IDENT_FIELDS.index(f) for f in ("CYdr", "Cndr", "Cldr")]
    assert np.all(r["params"][ref.IDX[rud]] == kp[ref.IDX[rud]])
    others = [j for j in range(21) if j not in rud]
    err = float(np.abs((r["params"][ref.IDX] - truth[ref.IDX]) / ref.scales(kp))[others].max())
    print(f"rudder 0: others recovered to {err:.2e}")
    assert err <= 1e-10


def _pg_ratio(kp, X, U, cfg, r):
    lo, hi = -np.array(list(cfg.lb_rel)), np.array(list(cfg.ub_rel))
    _, g0, _ = ref.normal(kp, kp[ref.IDX], X, U, cfg)
    _, g1, _ = ref.normal(kp, r["params"][ref.IDX], X, U, cfg)
    p0 = np.abs(ref.projected_gradient(np.zeros(21), g0, lo, hi)).max()
    p1 = np.abs(ref.projected_gradient(r["z"], g1, lo, hi)).max()
    return p1 / p0


def test_truth_outside_the_box(kp, x0):
    truth = _truth(kp, 13)
    T = 16
    U = ref.controls(T, H, 5)
    X = ref.make_log(truth, x0, U, H, SUB)
    cfg = _cfg(lb_rel=0.05, ub_rel=0.05, iters=12)
    r = ref.identify(kp, X, U, cfg)
    assert all(b <= a for a, b in zip(r["costs"], r["costs"][1:]))
    ratio = _pg_ratio(kp, X, U, cfg, r)
    print(f"box 5 %: projected gradient ratio {ratio:.2e}, status {r['status']}")
    assert ratio <= 1e-9
    assert np.all(r["z"] >= -0.05) and np.all(r["z"] <= 0.05)
    assert r["status"] & ok.IDENT_AT_BOUND


@pytest.mark.parametrize("L", [1, 4])
def test_noisy_log_reaches_a_stationary_point(kp, x0, L):
    truth = _truth(kp, 14)
    T = 40
    U = ref.controls(T, H, 6)
    X = ref.make_log(truth, x0, U, H, SUB)
    X = X + 1e-3 * np.random.default_rng(7).normal(size=X.shape)
    cfg = _cfg(lb_rel=0.5, ub_rel=0.5, iters=12, segment=L)
    r = ref.identify(kp, X, U, cfg)
    ratio = _pg_ratio(kp, X, U, cfg, r)
    print(f"noise 1e-3, L={L}: projected gradient ratio {ratio:.2e}")
    assert ratio <= 1e-6
    assert all(b <= a for a, b in zip(r["costs"], r["costs"][1:]))


# ---- round trips of the host-only surface ------------------------------------
def test_default_config_is_the_reference():
    c = ok.ident_default_config()
    assert (c.substeps, c.segment, c.iters) == (4, 1, 12)
    assert (c.h, c.alpha, c.lm0, c.tol) == (0.02, 0.0, 1e-6, 1e-10)
    assert list(c.Q) == [1e3, 1e2, 1e2, 1e2, 1e2, 1e2, 1e1, 1e1, 1e2, 1e2, 1e2, 1e2, 1e2]
    # kite_identification_test.cpp:127-148
    assert list(c.lb_rel) == [0.1, 0.05, 0.1, 0.5, 0.5, 0.1, 0.5, 0.5, 0.2, 0.3, 0.3, 0.5, 0.5, 0.5, 0.5, 0.3,
                              0.5, 0.5, 0.5, 0.5, 0.5]
    assert list(c.ub_rel) == [0.1, 0.1, 0.25, 0.5, 0.5, 0.3, 0.5, 0.5, 0.2, 0.3, 0.3, 0.5, 0.5, 0.5, 0.5, 1.0,
                              0.5, 0.5, 0.5, 0.5, 0.5]


def test_param_index_is_consistent_with_ident_fields():
    assert ok.IDENT_FIELDS == ref.IDENT_FIELDS and len(ok.IDENT_FIELDS) == ok.IDENT_NP == 21
    names = [f for f, _ in ok.KiteParams._fields_]
    for j, f in enumerate(ok.IDENT_FIELDS):
        assert ok.ident_param_index(j) == names.index(f) == ref.IDX[j]
    assert ok.ident_param_index(-1) == -1 and ok.ident_param_index(21) == -1


def test_save_properties_round_trip_is_bitwise(tmp_path, kp):
    row = ok.perturb_params(kp, 1, 0.1, 99)[0]
    row[49:52] = [0.01, -1e-300, 3.0e-7]
    f = tmp_path / "umx_radian_id.yaml"
    ok.save_properties(str(f), row)
    back = ok.load_properties(str(f)).as_array()
    assert back.tobytes() == row.tobytes()
    ok.save_properties(str(f), ok.load_properties())
    assert ok.load_properties(str(f)).as_array().tobytes() == kp.tobytes()


def test_ident_config_layout_matches_c_compiler(tmp_path):
    S = ok.IdentConfig
    fields = [f for f, _ in S._fields_]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kite_nmpc/kite_nmpc.h"\nint main(void){'
                   + 'printf("%zu\\n", sizeof(kite_ident_config));'
                   + "".join(f'printf("%zu\\n", offsetof(kite_ident_config, {f}));' for f in fields) + "return 0;}")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ok.nmpc.REPO, "include"), "-o", str(exe), str(src)],
                   check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(S)
    assert out[1:] == [getattr(S, f).offset for f in fields]


def test_workspace_and_validation_are_host_side():
    """Argument validation needs no device: the workspace size refuses what
    kite_nmpc_identify refuses."""
    c = ok.ident_default_config()
    n = ok.ident_workspace_doubles(c, 4, 20)
    assert n == 4 * 320 + 4 * 3 * 256                       # state + 3 chunks of KITE_IDENT_CHUNK samples
    assert ok.IDENT_CHUNK == 8
    for bad in (dict(substeps=0), dict(substeps=65), dict(segment=0), dict(segment=21), dict(iters=0), dict(iters=65),
                dict(h=0.0), dict(h=math.nan), dict(alpha=-1.0), dict(lm0=math.inf), dict(tol=-1e-3),
                dict(Q=[-1.0] + [1.0] * 12), dict(lb_rel=[-0.1] + [0.1] * 20)):
        with pytest.raises(ok.KiteNmpcError) as e:
            ok.ident_workspace_doubles(ok.ident_default_config(**bad), 4, 20)
        assert e.value.code == ok.nmpc.KITE_EINVAL, bad
    for T in (0, (1 << 20) + 1):
        with pytest.raises(ok.KiteNmpcError):
            ok.ident_workspace_doubles(c, 4, T)
