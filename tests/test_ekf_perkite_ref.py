"""CPU side of the per-kite estimator models (kite_nmpc_set_estimator_model,
k_ekf_pk, k_ekf_wind_pk): the ABI is there, and the per-kite references the GPU
tests compare against (tests/ekf_perkite_cases.py) separate a filter that uses
each kite's row from one that ignores the rows.

  * One step: each kite's reference under its own row is at least GAP = 1e3
    parity bars away from its reference under the nominal row, for both
    filters, with and without the update (B = 9, the filter inputs of
    test_wind_ekf.py, the library's default covariances).  Measured here, in
    bars per kite: k_ekf x 2.2e10 .. 8.7e10 and P 2.4e10 .. 1.9e11 (both
    without and with the update); the wind filter's x13 7.1e9 .. 1.2e11
    (propagation alone), 2.2e10 .. 1.1e11 (with the update).
  * Open loop (test_wind_ekf.py's run with the truth integrated under
    rows_for(8)): with each kite's own row the reference filter ends at a
    wind-error ratio <= 0.25 on every kite, with the nominal row at least one
    kite ends above it.  Measured here with the library's default covariances
    and the run's own seed 42 (no other seed was tried): own rows 0.078 0.100
    0.123 0.191 0.116 0.048 0.169 0.096, nominal row 0.096 0.210 0.057 0.219
    0.546 0.122 0.225 0.077.
"""
import inspect

import numpy as np
import pytest

import openkite_amd as ok
from openkite_amd import fleet, nmpc
from tests import ekf_perkite_cases as ec

B9 = 9


def test_symbols_and_wrappers_exist():
    L = ok.lib()
    for name in ("kite_nmpc_set_estimator_model", "kite_nmpc_get_estimator_model"):
        assert hasattr(L, name), name
        assert name in nmpc._SIGNATURES
    assert callable(ok.BatchNMPC.set_estimator_model)
    assert isinstance(ok.BatchNMPC.estimator_model, property)
    assert callable(fleet.GpuStepper.set_estimator_model)
    assert inspect.signature(fleet.FleetLoop.__init__).parameters["estimator_model"].default == "creation"
    assert (ok.EST_MODEL_CREATION, ok.EST_MODEL_CONTROLLER) == (0, 1)
    assert L.kite_nmpc_api_version() == 7                  # additive


def test_null_context_is_refused():
    import ctypes
    L = ok.lib()
    m = ctypes.c_int32(5)
    assert L.kite_nmpc_set_estimator_model(None, 1) == nmpc.KITE_EINVAL
    assert L.kite_nmpc_get_estimator_model(None, ctypes.byref(m)) == nmpc.KITE_EINVAL
    assert m.value == 5


def test_fleet_loop_refuses_a_controller_model_without_an_estimator():
    import torch
    x0 = torch.zeros((2, 15), dtype=torch.float64)
    with pytest.raises(ValueError):
        fleet.FleetLoop(None, x0, 20, 0.05, estimator_model="controller")
    with pytest.raises(ValueError):
        fleet.FleetLoop(None, x0, 20, 0.05, estimator_model="nominal")
    # "creation" calls nothing on the stepper: a loop without one still constructs
    fleet.FleetLoop(None, x0, 20, 0.05)


@pytest.mark.parametrize("update", [False, True])
def test_ekf_reference_is_sensitive_to_the_rows(update):
    own = ec.ekf_reference(B9, 1, update, True)
    nom = ec.ekf_reference(B9, 1, update, False)
    gx = ec.worst_per_kite(nom[0], own[0], ec.X_RTOL)
    gP = ec.worst_per_kite(nom[1], own[1], ec.P_RTOL)
    print(f"k_ekf, update {update}: own row vs nominal row in parity bars per kite: x {np.array2string(gx, precision=2)}"
          f" P {np.array2string(gP, precision=2)}")
    assert np.all(gx >= ec.GAP) and np.all(gP >= ec.GAP)


@pytest.mark.parametrize("update", [False, True])
def test_wind_reference_is_sensitive_to_the_rows(update):
    own = ec.wind_reference(B9, 1, update, True)
    nom = ec.wind_reference(B9, 1, update, False)
    gx = ec.worst_per_kite(nom[0][:, :13], own[0][:, :13], ec.X_RTOL)
    print(f"wind filter, update {update}: x13 own row vs nominal row in parity bars per kite: "
          f"{np.array2string(gx, precision=2)}")
    assert np.all(gx >= ec.GAP)


def test_open_loop_needs_each_kites_own_row():
    own = ec.wind_error_ratio(ec.open_loop_reference(True)[0])
    nom = ec.wind_error_ratio(ec.open_loop_reference(False)[0])
    print("final / initial wind error, own rows in the filter:", np.round(own, 3))
    print("final / initial wind error, the nominal row in the filter:", np.round(nom, 3))
    assert np.all(own <= 0.25), own
    assert np.any(nom > 0.25), nom
