"""CPU tests of the per-kite controller models (kite_nmpc_set_params,
_set_params_device, _get_params): the ABI is there, and the oracle reference
the GPU tests compare against is sensitive to the rows -- a controller that
ignored them would miss it by three orders of magnitude more than the parity
bar allows."""
import inspect

import numpy as np

import openkite_amd as ok
from openkite_amd import fleet, nmpc
from tests import perkite_cases as pc
from tests.test_gpu_parity import COND_ENVELOPE, MS_ENVELOPE


def test_symbols_and_wrappers_exist():
    L = ok.lib()
    for name in ("kite_nmpc_set_params", "kite_nmpc_set_params_device", "kite_nmpc_get_params"):
        assert hasattr(L, name), name
        assert name in nmpc._SIGNATURES
    for name in ("set_params", "set_params_device", "get_params"):
        assert callable(getattr(ok.BatchNMPC, name))
    assert callable(fleet.GpuStepper.set_params_device)
    assert "adapt" in inspect.signature(fleet.FleetLoop.__init__).parameters
    assert nmpc.PARAMS_REJECTED == 1
    assert ok.lib().kite_nmpc_api_version() == 7          # additive


def test_null_context_is_refused():
    L = ok.lib()
    row = ok.load_properties().as_array()
    assert L.kite_nmpc_set_params(None, row.ctypes.data, 1) == nmpc.KITE_EINVAL
    assert L.kite_nmpc_set_params_device(None, None, 1, None) == nmpc.KITE_EINVAL
    assert L.kite_nmpc_get_params(None, row.ctypes.data) == nmpc.KITE_EINVAL


def test_rows_are_heterogeneous():
    rows = pc.rows_for(pc.B9)
    kp = ok.load_properties().as_array()
    f = nmpc._PARAM_FIELDS
    idx = [f.index(n) for n in ok.IDENT_FIELDS]
    assert np.all(np.abs(rows[:, idx] / kp[idx] - 1.0) <= 0.10 + 1e-15)
    assert np.all(np.abs(rows[:, idx] / kp[idx] - 1.0).max(1) > 0.05)
    assert rows[1, f.index("mass")] != kp[f.index("mass")] and rows[2, f.index("Ixx")] != kp[f.index("Ixx")]
    other = [i for i in range(52) if i not in idx and f[i] not in ("mass", "Ixx")]
    np.testing.assert_array_equal(rows[:, other], np.repeat(kp[None, other], pc.B9, axis=0))


def _gaps(Nh, B, steps, offset, bar):
    loop = pc.oracle_loop(Nh, B, steps, offset)
    nom = pc.oracle_nominal(Nh, B, steps, offset)
    for step in sorted(nom):
        _, u0, X, U, _, _ = loop[step]
        gap = pc.plan_gap(u0, X, U, nom[step])
        sat = np.abs(u0 - nom[step][0]).max(1)
        print(f"N = {Nh}, step {step}: plan gap own row vs nominal row, per kite: {np.array2string(gap, precision=2)}; "
              f"of u0 alone: {' '.join('%.1e' % v for v in sat)}")
        assert np.all(gap >= pc.GAP * bar), (Nh, step, gap)


def test_oracle_is_sensitive_to_the_rows_n20():
    """Cold step and third warm step at N = 20, B = 9 (the cases of the GPU
    parity test): every kite's oracle plan under its own row is >= 1e3 x
    COND_ENVELOPE -- the bar every kite of assert_cond_rti must meet -- away
    from the oracle under the nominal row, in assert_cond_rti's own measure
    (the largest of u0, trajectory, controls per kite).  u0 alone cannot carry
    this: from the synthetic states the first control sits on its bounds under
    either row (thrust, elevator, rudder and mostly Uv; printed above), so the
    gap is taken over what the parity bars compare."""
    _gaps(20, pc.B9, 6, 9100, COND_ENVELOPE)


def test_oracle_is_sensitive_to_the_rows_n40():
    """The same at N = 40, B = 3 (cold step and second warm step: the GPU loop
    there is cold + 2), against assert_ms_rti's MS_ENVELOPE."""
    _gaps(40, 3, 3, 9140, MS_ENVELOPE)
