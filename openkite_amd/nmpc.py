"""Python host side of the MI355X kite NMPC: ctypes binding of the C ABI
(include/kite_nmpc/kite_nmpc.h) plus a ``KiteNMPF`` class that mirrors the
reference controller API (src/kite_control/kiteNMPF.h:10-118).

Every numerical call goes to libkite_nmpc.so on the GPU; if the library is
missing or no gfx950 device is present the calls raise -- there is no CPU
fallback.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KITE_NMPC_LIB", os.path.join(_HERE, "lib", "libkite_nmpc.so"))
REPO = os.path.dirname(_HERE)
DEFAULT_PARAMS = os.path.join(REPO, "data", "umx_radian.yaml")

KITE_OK, KITE_EINVAL, KITE_EHIP, KITE_ENOMEM, KITE_ENODEV, KITE_EIO, KITE_EPARSE, KITE_ESTATE = 0, -1, -2, -3, -4, -5, -6, -7
ST_NAN, ST_QP_NOT_CONV, ST_MIN_SPEED, ST_STATE_BOUND, ST_THETA_WRAP, ST_STEP_REJECTED = 1, 2, 4, 8, 16, 32
ST_RESTART = 64
ST_BAD_INFLIGHT = 128              # KITE_ST_BAD_INFLIGHT: the kite's in-flight schedule row is invalid
INFLIGHT_N = 24                    # KITE_INFLIGHT_N: doubles per kite of the in-flight schedule
PLANT_NAN = 1                      # KITE_PLANT_NAN (plant status word)
PLANT_CMD_DROPPED, PLANT_BAD_TAU = 2, 4    # KITE_PLANT_* of the delayed step: oldest command dropped, bad latency
# the command line of plant_step_delayed (KITE_DELAY_*): depth, doubles per kite and the slots
DELAY_DEPTH, DELAY_NLINE = 4, 32
DELAY_COUNT, DELAY_T_PREV, DELAY_HAS_PREV, DELAY_U_FORCE, DELAY_T_ARR, DELAY_U = 0, 1, 2, 4, 8, 12
# the line's arrival rule (slot DELAY_RULE): sequential, t_arr = max(t_send, t_arr_prev) + tau, or
# transport, t_arr = max(t_send + tau, t_arr_prev); exactly 1.0 in the slot is transport, anything else sequential
DELAY_RULE, DELAY_RULE_SEQUENTIAL, DELAY_RULE_TRANSPORT = 3, 0, 1
EKF_NAN, EKF_S_NOT_PD = 1, 2       # KITE_EKF_* (status word of the wind-estimating and the kinematic EKF)
EKF_INIT_BAD = 4                   # KITE_EKF_INIT_BAD (status word of kin_ekf_init)
WIND_MAX_DEFAULT = 20.0            # set_wind_device: clamp of an estimated wind component, m/s
IDENT_NAN, IDENT_CONVERGED, IDENT_AT_BOUND = 1, 2, 4   # KITE_IDENT_* (status word of the identification)
IDENT_WIND_AT_BOUND = 8            # KITE_IDENT_WIND_AT_BOUND (joint identification: the wind ends on its box)
IDENT_NPW = 24                     # KITE_IDENT_NPW: the 21 and the wind offset
PARAMS_REJECTED = 1                # KITE_PARAMS_REJECTED (status word of set_params_device)
QP_SPLIT_AUTO = -1                 # KITE_QP_SPLIT_*: the two-phase tiled QP (set_qp_split)
QP_SPLIT_NEVER = 0
EST_MODEL_CREATION = 0             # KITE_EST_MODEL_*: the model of the two EKFs (set_estimator_model)
EST_MODEL_CONTROLLER = 1
IDENT_NP = 21                      # KITE_IDENT_NP
IDENT_CHUNK = 8                    # KITE_IDENT_CHUNK: samples per partial sum of k_ident_accum
# closed-loop scoring (KITE_SCORE_*): doubles per kite in acc / mem, doubles of the summary, and the slots
SCORE_NACC, SCORE_NSUM, SCORE_NMEM = 16, 16, 8
(SCORE_N, SCORE_N_LOST, SCORE_EVER_LOST, SCORE_SUM_D2, SCORE_MAX_D, SCORE_SUM_TRACK, SCORE_SUM_U, SCORE_SUM_RATE,
 SCORE_SUM_SPEED, SCORE_MIN_SPEED, SCORE_PROGRESS, SCORE_N_MIN_SPEED, SCORE_N_QP_NOT_CONV, SCORE_N_STATE_BOUND,
 SCORE_N_RATE, SCORE_SPARE) = range(16)
SCORE_KITES = 15                   # summary only: the number of rows reduced
SCORE_MEM_THETA, SCORE_MEM_U, SCORE_MEM_VALID = 0, 1, 5
# names of the acc slots (the summary's slot 15 is "kites")
SCORE_SLOTS = ["n", "n_lost", "ever_lost", "sum_d2", "max_d", "sum_track", "sum_u", "sum_rate", "sum_speed",
               "min_speed", "progress", "n_min_speed", "n_qp_not_conv", "n_state_bound", "n_rate", "spare"]
# the identified parameters in the reference's REF_P order (kite_identification_test.cpp:120-121)
IDENT_FIELDS = ["CL0", "CLa_total", "CD0_total", "CYb", "Cm0", "Cma", "Cnb", "Clb", "CLq", "Cmq",
                "CYr", "Cnr", "Clr", "CYp", "Clp", "Cnp", "CLde", "CYdr", "Cmde", "Cndr", "Cldr"]

_PARAM_FIELDS = ["b", "c", "AR", "S", "lam", "St", "lt", "Sf", "lf", "Xac",
                 "mass", "Ixx", "Iyy", "Izz", "Ixz",
                 "CL0", "CL0_tail", "CLa_total", "CLa_wing", "CLa_tail", "e_oswald",
                 "CD0_total", "CD0_wing", "CD0_tail", "CYb", "CYb_vtail", "Cm0", "Cma",
                 "Cn0", "Cnb", "Cl0", "Clb", "CLq", "Cmq", "CYr", "Cnr", "Clr", "CYp", "Clp", "Cnp",
                 "CLde", "CYdr", "Cmde", "Cndr", "Cldr", "CDde",
                 "Lt", "Ks", "Kd", "rx", "ry", "rz"]


class KiteParams(ctypes.Structure):
    """kite_params (KiteProperties flattened, kite.h:9-93)."""
    _fields_ = [(f, ctypes.c_double) for f in _PARAM_FIELDS]

    def as_array(self) -> np.ndarray:
        return np.array([getattr(self, f) for f in _PARAM_FIELDS], dtype=np.float64)


PATH_HMAX = 8                      # KITE_PATH_MAX_HARMONICS
PATH_NC = 2 * PATH_HMAX + 1


class NmpcConfig(ctypes.Structure):
    _fields_ = [
        ("N", ctypes.c_int32), ("M", ctypes.c_int32), ("qp_iters", ctypes.c_int32), ("shift", ctypes.c_int32),
        ("device", ctypes.c_int32), ("timing", ctypes.c_int32), ("qp_kernel", ctypes.c_int32),
        ("delay_steps", ctypes.c_int32),
        ("dt", ctypes.c_double), ("Q", ctypes.c_double * 3), ("R", ctypes.c_double * 4), ("W", ctypes.c_double),
        ("Sx", ctypes.c_double * 15), ("Su", ctypes.c_double * 4),
        ("lbx", ctypes.c_double * 15), ("ubx", ctypes.c_double * 15),
        ("lbu", ctypes.c_double * 4), ("ubu", ctypes.c_double * 4),
        ("vref", ctypes.c_double), ("path_radius", ctypes.c_double), ("path_altitude", ctypes.c_double),
        ("path_q", ctypes.c_double * 4), ("theta_flex", ctypes.c_double), ("min_speed", ctypes.c_double),
        ("delay", ctypes.c_double),
        ("sens_fp32", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("qp_soft_weight", ctypes.c_double), ("qp_lm", ctypes.c_double),
        ("path_harmonics", ctypes.c_int32), ("reserved2", ctypes.c_int32),
        ("path_fourier", ctypes.c_double * (3 * PATH_NC)),   # [3][2 * 8 + 1], row-major
    ]

    def set_fourier_path(self, coef, q=None) -> None:
        """Arbitrary closed path (KiteNMPF(kite, path), kiteNMPF.h:14): coef is
        (3, 2K + 1) per axis [c0, a1, b1, ..., aK, bK] of the unrotated curve
        p_a(theta) = c0 + sum_k a_k cos(k theta) + b_k sin(k theta), K <= 8;
        P = rot(q) p as for the circle (q None: keep path_q)."""
        c = np.asarray(coef, dtype=np.float64)
        if c.ndim != 2 or c.shape[0] != 3 or c.shape[1] % 2 != 1 or not 3 <= c.shape[1] <= PATH_NC:
            raise ValueError("coef must be (3, 2K+1) with 1 <= K <= %d" % PATH_HMAX)
        F = np.zeros((3, PATH_NC))
        F[:, :c.shape[1]] = c
        self.path_harmonics = (c.shape[1] - 1) // 2
        for i, v in enumerate(F.reshape(-1)):
            self.path_fourier[i] = v
        if q is not None:
            for i in range(4):
                self.path_q[i] = q[i]

    def to_dict(self) -> dict:
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if hasattr(v, "__len__") else v
        return d


class CollocConfig(ctypes.Structure):
    """kite_colloc_config: the reference's collocation NLP functions (chebyshev.hpp)."""
    _fields_ = [
        ("poly_order", ctypes.c_int32), ("num_segments", ctypes.c_int32), ("use_R", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("t0", ctypes.c_double), ("tf", ctypes.c_double), ("Q", ctypes.c_double * 3), ("R", ctypes.c_double * 4),
        ("W", ctypes.c_double), ("vref", ctypes.c_double), ("mayer_scale", ctypes.c_double),
        ("Sx", ctypes.c_double * 15), ("Su", ctypes.c_double * 4),
        ("path_radius", ctypes.c_double), ("path_altitude", ctypes.c_double), ("path_q", ctypes.c_double * 4),
        ("path_harmonics", ctypes.c_int32), ("reserved2", ctypes.c_int32),
        ("path_fourier", ctypes.c_double * (3 * PATH_NC)),
    ]

    def to_dict(self) -> dict:
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if hasattr(v, "__len__") else v
        return d


class IdentConfig(ctypes.Structure):
    """kite_ident_config: the identification of the 21 aerodynamic coefficients."""
    _fields_ = [
        ("substeps", ctypes.c_int32), ("segment", ctypes.c_int32), ("iters", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("h", ctypes.c_double), ("Q", ctypes.c_double * 13), ("alpha", ctypes.c_double), ("lm0", ctypes.c_double),
        ("tol", ctypes.c_double), ("lb_rel", ctypes.c_double * 21), ("ub_rel", ctypes.c_double * 21),
    ]

    def to_dict(self) -> dict:
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if hasattr(v, "__len__") else v
        return d


class IdentWindConfig(ctypes.Structure):
    """kite_ident_wind_config: the wind variables of the joint identification."""
    _fields_ = [("w_scale", ctypes.c_double), ("w_prior", ctypes.c_double * 3), ("w_box", ctypes.c_double * 3),
                ("alpha_w", ctypes.c_double)]

    def to_dict(self) -> dict:
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if hasattr(v, "__len__") else v
        return d


class PoseFrame(ctypes.Structure):
    """kite_pose_frame: the motion-capture -> world change of a measured pose
    (optitrack2world, ekf_node.cpp:148-169)."""
    _fields_ = [("offset", ctypes.c_double * 3), ("rotation", ctypes.c_double * 4), ("shift", ctypes.c_double * 3)]

    def to_dict(self) -> dict:
        return {name: tuple(getattr(self, name)) for name, _ in self._fields_}


def _frame(frame):
    """A ``PoseFrame`` (or a dict of its three fields) as the C argument; None stays NULL."""
    if frame is None:
        return None
    if not isinstance(frame, PoseFrame):
        frame = PoseFrame(*(tuple(float(v) for v in frame[k]) for k in ("offset", "rotation", "shift")))
    return ctypes.byref(frame)


class MpcDiagnostic(ctypes.Structure):
    """msg/mpc_diagnostic.msg field order."""
    _fields_ = [("pos_error", ctypes.c_double), ("vel_error", ctypes.c_double), ("cost", ctypes.c_double),
                ("virt_state", ctypes.c_double), ("virt_ctrl", ctypes.c_double), ("comp_time_ms", ctypes.c_double)]


DIAG_FIELDS = [f for f, _ in MpcDiagnostic._fields_]

_lib = None
_DP = ctypes.POINTER(ctypes.c_double)
_IP = ctypes.POINTER(ctypes.c_int32)

# every symbol of include/kite_nmpc/kite_nmpc.h with its ctypes signature
_SIGNATURES = {
    "kite_nmpc_api_version": (ctypes.c_int, []),
    "kite_nmpc_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "kite_params_load_yaml": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(KiteParams)]),
    "kite_nmpc_default_config": (None, [ctypes.POINTER(NmpcConfig)]),
    "kite_nmpc_create": (ctypes.c_int, [ctypes.POINTER(KiteParams), ctypes.POINTER(NmpcConfig), ctypes.c_int32,
                                        ctypes.POINTER(ctypes.c_void_p)]),
    "kite_nmpc_destroy": (None, [ctypes.c_void_p]),
    "kite_nmpc_batch": (ctypes.c_int, [ctypes.c_void_p]),
    "kite_nmpc_set_bounds": (ctypes.c_int, [ctypes.c_void_p, _DP, _DP, _DP, _DP]),
    "kite_nmpc_set_reference_velocity": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double]),
    "kite_nmpc_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "kite_nmpc_set_wind": (ctypes.c_int, [ctypes.c_void_p, _DP]),
    "kite_nmpc_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "kite_nmpc_use_own_stream": (ctypes.c_int, [ctypes.c_void_p]),
    "kite_nmpc_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "kite_nmpc_closest_point": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP]),
    "kite_nmpc_path_eval": (ctypes.c_int, [ctypes.POINTER(NmpcConfig), ctypes.c_int32, _DP, _DP, _DP]),
    "kite_nmpc_step": (ctypes.c_int, [ctypes.c_void_p, _DP, _DP, _DP, _DP, ctypes.POINTER(MpcDiagnostic), _IP]),
    "kite_nmpc_step_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kite_nmpc_get_solution": (ctypes.c_int, [ctypes.c_void_p, _DP, _DP]),
    "kite_nmpc_set_solution": (ctypes.c_int, [ctypes.c_void_p, _DP, _DP]),
    "kite_nmpc_dynamics": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP]),
    "kite_nmpc_jacobian": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, _DP]),
    "kite_nmpc_predict": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _DP, _DP, ctypes.c_double,
                                         ctypes.c_int32, _DP]),
    "kite_nmpc_rk4_sens": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _DP, _DP, ctypes.c_double,
                                          ctypes.c_int32, _DP, _DP, _DP]),
    "kite_nmpc_kernel_times": (ctypes.c_int, [ctypes.c_void_p, _DP, ctypes.c_int32]),
    "kite_nmpc_get_qp": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, _DP, _DP]),
    "kite_nmpc_timing_start": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "kite_nmpc_timing_start_sampled": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]),
    "kite_nmpc_timing_read": (ctypes.c_int, [ctypes.c_void_p, _DP, ctypes.c_int32]),
    "kite_nmpc_qp_stats": (ctypes.c_int, [ctypes.c_void_p, _DP, _IP]),
    "kite_nmpc_qp_iteration_sum": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    "kite_nmpc_state_bound_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                                   ctypes.POINTER(ctypes.c_int64)]),
    "kite_ekf_default_covariances": (None, [_DP, _DP, _DP]),
    "kite_colloc_default_config": (None, [ctypes.c_void_p]),
    "kite_nmpc_colloc_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, _DP]),
    "kite_nmpc_ekf_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, _DP, _DP, _DP, _DP,
                                          _DP, _DP]),
    "kite_nmpc_ekf_step_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "kite_windekf_default_covariances": (None, [_DP, _DP, _DP]),
    "kite_nmpc_windekf_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, _DP,
                                              _DP, _DP, _DP, _DP, _DP, _IP]),
    "kite_nmpc_windekf_step_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p]),
    "kite_nmpc_jacobian_wind": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, _DP]),
    "kite_nmpc_set_wind_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_double]),
    "kite_pose_frame_default": (None, [ctypes.POINTER(PoseFrame)]),
    "kite_nmpc_kinekf_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32, _DP,
                                             _DP, _DP, _DP, _DP, ctypes.POINTER(PoseFrame), _IP]),
    "kite_nmpc_kinekf_step_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(PoseFrame),
                                                    ctypes.c_void_p]),
    "kite_nmpc_kinekf_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, _DP, _DP,
                                             ctypes.POINTER(PoseFrame), _DP, _IP]),
    "kite_nmpc_kinekf_init_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(PoseFrame),
                                                    ctypes.c_void_p, ctypes.c_void_p]),
    "kite_nmpc_jacobian_kin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _DP, _DP]),
    "kite_nmpc_set_params": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]),
    "kite_nmpc_set_params_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]),
    "kite_nmpc_get_params": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "kite_nmpc_set_estimator_model": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "kite_nmpc_get_estimator_model": (ctypes.c_int, [ctypes.c_void_p, _IP]),
    "kite_nmpc_set_qp_split": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "kite_nmpc_get_qp_split": (ctypes.c_int, [ctypes.c_void_p, _IP, _IP, _IP, ctypes.POINTER(ctypes.c_int64)]),
    "kite_ident_default_config": (None, [ctypes.POINTER(IdentConfig)]),
    "kite_ident_param_index": (ctypes.c_int, [ctypes.c_int32]),
    "kite_nmpc_ident_sens": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, _DP]),
    "kite_nmpc_ident_normal": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IdentConfig), ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, _DP, _DP,
                                              _DP, _IP]),
    "kite_nmpc_identify": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IdentConfig), ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_void_p, ctypes.c_int32, _DP, _DP, ctypes.c_void_p, _DP, _IP, _IP]),
    "kite_nmpc_identify_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IdentConfig), ctypes.c_int32,
                                                 ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
    "kite_nmpc_ident_workspace_doubles": (ctypes.c_int64, [ctypes.POINTER(IdentConfig), ctypes.c_int32,
                                                           ctypes.c_int32]),
    "kite_nmpc_ident_sens_wind": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32,
                                                 ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, _DP, _DP]),
    "kite_nmpc_ident_normal_wind": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IdentConfig), ctypes.c_int32,
                                                   ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, _DP,
                                                   _DP, _DP, _DP, _IP]),
    "kite_nmpc_identify_wind": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IdentConfig), ctypes.c_int32,
                                               ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP,
                                               ctypes.c_void_p, _DP, _IP, _IP]),
    "kite_nmpc_identify_wind_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IdentConfig), ctypes.c_int32,
                                                      ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_void_p]),
    "kite_ident_wind_default_config": (None, [ctypes.POINTER(IdentWindConfig)]),
    "kite_nmpc_ident_sens_joint": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_int32,
                                                  ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, _DP, _DP]),
    "kite_nmpc_ident_normal_joint": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IdentConfig),
                                                    ctypes.POINTER(IdentWindConfig), ctypes.c_int32, ctypes.c_int32,
                                                    ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, _DP, _DP, _DP, _DP,
                                                    _DP, _IP]),
    "kite_nmpc_identify_joint": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IdentConfig),
                                                ctypes.POINTER(IdentWindConfig), ctypes.c_int32, ctypes.c_int32,
                                                ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP, ctypes.c_void_p, _DP,
                                                _DP, _IP, _IP]),
    "kite_nmpc_identify_joint_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(IdentConfig),
                                                       ctypes.POINTER(IdentWindConfig), ctypes.c_int32, ctypes.c_int32,
                                                       ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_void_p]),
    "kite_nmpc_ident_joint_workspace_doubles": (ctypes.c_int64, [ctypes.POINTER(IdentConfig), ctypes.c_int32,
                                                                 ctypes.c_int32]),
    "kite_nmpc_plant_set_params": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]),
    "kite_nmpc_plant_set_wind": (ctypes.c_int, [ctypes.c_void_p, _DP]),
    "kite_nmpc_plant_step": (ctypes.c_int, [ctypes.c_void_p, _DP, _DP, ctypes.c_double, ctypes.c_double,
                                            ctypes.c_int32, ctypes.c_int32, _IP]),
    "kite_nmpc_plant_step_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int32,
                                                   ctypes.c_void_p]),
    "kite_nmpc_plant_step_delayed": (ctypes.c_int, [ctypes.c_void_p, _DP, _DP, _DP, _DP, _DP, ctypes.c_double,
                                                    ctypes.c_double, ctypes.c_int32, ctypes.c_int32, _IP]),
    "kite_nmpc_plant_step_delayed_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                           ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                                           ctypes.c_int32, ctypes.c_void_p]),
    "kite_nmpc_set_inflight": (ctypes.c_int, [ctypes.c_void_p, _DP, ctypes.c_double]),
    "kite_nmpc_set_inflight_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double]),
    "kite_nmpc_get_inflight": (ctypes.c_int, [ctypes.c_void_p, _DP]),
    "kite_nmpc_closest_point_global": (ctypes.c_int,[ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _DP]),
    "kite_nmpc_closest_point_global_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                             ctypes.c_void_p, ctypes.c_void_p]),
    "kite_nmpc_score_step": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _DP, _DP, _IP, _IP, ctypes.c_int32,
                                            _DP, _DP]),
    "kite_nmpc_score_step_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                   ctypes.c_void_p]),
    "kite_nmpc_score_summary": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _DP, _DP]),
    "kite_nmpc_score_summary_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                      ctypes.c_void_p]),
}


class KiteNmpcError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        msg = lib().kite_nmpc_strerror(code).decode() if _lib is not None else str(code)
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")
        self.code = code


def lib():
    """Load libkite_nmpc.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: build it with `make -C openkite_amd/csrc` "
                               "(or __graft_entry__.build()); there is no CPU fallback")
        # One HIP runtime per process.  PyTorch-ROCm ships its own
        # libamdhip64 (SONAME libamdhip64.so.7) and NEEDs it by the unversioned
        # name: if /opt/rocm's copy is mapped first, torch maps a second one
        # and sees no GPU (and torch stream handles mean nothing to ours).
        # Mapping torch first makes our NEEDED libamdhip64.so.7 bind to it.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(code: int, what: str):
    if code < 0:
        raise KiteNmpcError(code, what)
    return code


def _p(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], "float64 C-contiguous array required"
    return a.ctypes.data_as(_DP)


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def load_properties(path: str = DEFAULT_PARAMS) -> KiteParams:
    """kite_utils::LoadProperties (kite.cpp:7-76) via the C ABI."""
    p = KiteParams()
    _check(lib().kite_params_load_yaml(path.encode(), ctypes.byref(p)), f"load {path}")
    return p


# YAML keys of the 52 fields (kite_utils::LoadProperties, kite.cpp:7-76): the
# field names in their sections, the tether length under its own key
_YAML_SECTIONS = (("geometry", 0, 10), ("inertia", 10, 15), ("aerodynamic", 15, 46), ("tether", 46, 52))


def save_properties(path: str, params_row, template: str = DEFAULT_PARAMS) -> None:
    """Write a parameter file that ``load_properties`` reads back to the same 52
    doubles bit for bit (the reference's ``umx_radian_id.yaml`` step,
    kite_identification_test.cpp).  params_row: a ``KiteParams`` or 52 values;
    the top-level scalar lines of ``template`` (its ``name:``) are carried over."""
    v = params_row.as_array() if isinstance(params_row, KiteParams) else _f64(params_row).reshape(-1)
    if v.size != len(_PARAM_FIELDS):
        raise ValueError("52 parameter values expected")
    head = []
    if template:
        with open(template) as f:
            for line in f:
                body = line.split("#", 1)[0].rstrip()
                if body and not body[0].isspace() and ":" in body and body.split(":", 1)[1].strip():
                    head.append(body)
    out = ["# written by openkite_amd.save_properties"] + head
    for sec, lo, hi in _YAML_SECTIONS:
        out += ["", sec + ":"]
        for i in range(lo, hi):
            key = "length" if _PARAM_FIELDS[i] == "Lt" else _PARAM_FIELDS[i]
            out.append("    %s: %r" % (key, float(v[i])))     # repr round-trips through strtod
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


# perturb_params' default selection: what differs between two airframes of one
# design (mass, inertias, aerodynamic coefficients); the geometry (b .. Xac) and
# the tether (Lt .. rz) stay as they are
PERTURB_FIELDS = _PARAM_FIELDS[_PARAM_FIELDS.index("mass"):_PARAM_FIELDS.index("CDde") + 1]


def perturb_params(params, B: int, rel: float, seed: int, fields=None) -> np.ndarray:
    """A seeded fleet of B plant models around ``params`` (a ``KiteParams`` or
    its 52 values) for ``BatchNMPC.plant_set_params``: a (B, 52) array in which
    every selected field is multiplied by 1 + rel * U(-1, 1), one draw per kite
    and field from ``numpy.random.default_rng(seed)``.  fields: names from
    ``KiteParams`` (default ``PERTURB_FIELDS``); the others are copied."""
    base = params.as_array() if isinstance(params, KiteParams) else _f64(params).reshape(-1)
    if base.size != len(_PARAM_FIELDS):
        raise ValueError("52 parameter values expected")
    names = PERTURB_FIELDS if fields is None else list(fields)
    cols = [_PARAM_FIELDS.index(f) for f in names]      # ValueError on an unknown name
    out = np.repeat(base[None, :], int(B), axis=0)
    draws = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(int(B), len(cols)))
    out[:, cols] *= 1.0 + float(rel) * draws
    return out


def resolve_qp_kernel(qp_kernel: int, N: int) -> int:
    """The QP kernel a config selects (kite_nmpc_create): 0 (auto) is the
    register-tiled condensed QP (2) at N == 20, the multiple-shooting QP (3)
    otherwise."""
    return qp_kernel if qp_kernel else (2 if N == 20 else 3)


def default_config(**overrides) -> NmpcConfig:
    """The reference node's controller setup (nmpf_node.cpp:30-69) + RTI defaults."""
    c = NmpcConfig()
    lib().kite_nmpc_default_config(ctypes.byref(c))
    for k, v in overrides.items():
        if not hasattr(c, k):
            raise KeyError(k)
        cur = getattr(c, k)
        if hasattr(cur, "__len__"):
            for i, vi in enumerate(v):
                cur[i] = vi
        else:
            setattr(c, k, v)
    return c


def ident_default_config(**overrides) -> IdentConfig:
    """kite_ident_default_config: the reference's weights and boxes
    (kite_identification_test.cpp:127-148, :193), h = 0.02, 4 substeps, one-step
    segments, 12 evaluations."""
    c = IdentConfig()
    lib().kite_ident_default_config(ctypes.byref(c))
    for k, v in overrides.items():
        if not hasattr(c, k):
            raise KeyError(k)
        cur = getattr(c, k)
        if hasattr(cur, "__len__"):
            vv = np.broadcast_to(np.asarray(v, dtype=np.float64), (len(cur),))
            for i, vi in enumerate(vv):
                cur[i] = vi
        else:
            setattr(c, k, v)
    return c


def ident_param_index(j: int) -> int:
    """kite_params field index of identified parameter j (-1 outside 0..20)."""
    return int(lib().kite_ident_param_index(int(j)))


def ident_workspace_doubles(config: IdentConfig, count: int, T: int) -> int:
    """Workspace of ``BatchNMPC.identify_device`` in doubles."""
    return _check(int(lib().kite_nmpc_ident_workspace_doubles(ctypes.byref(config), int(count), int(T))),
                  "ident_workspace_doubles")


def ident_wind_default_config(**overrides) -> IdentWindConfig:
    """kite_ident_wind_default_config: w_scale 1 m/s, prior 0, box +-3 m/s, no prior weight."""
    c = IdentWindConfig()
    lib().kite_ident_wind_default_config(ctypes.byref(c))
    for k, v in overrides.items():
        if not hasattr(c, k):
            raise KeyError(k)
        cur = getattr(c, k)
        if hasattr(cur, "__len__"):
            vv = np.broadcast_to(np.asarray(v, dtype=np.float64), (len(cur),))
            for i, vi in enumerate(vv):
                cur[i] = vi
        else:
            setattr(c, k, v)
    return c


def ident_joint_workspace_doubles(config: IdentConfig, count: int, T: int) -> int:
    """Workspace of ``BatchNMPC.identify_joint_device`` in doubles."""
    return _check(int(lib().kite_nmpc_ident_joint_workspace_doubles(ctypes.byref(config), int(count), int(T))),
                  "ident_joint_workspace_doubles")


@dataclass
class IdentResult:
    """``BatchNMPC.identify``: params (B, 52) the input rows with the 21
    replaced, cost0 / cost the first and the final accepted cost, evals the
    evaluations done, status the KITE_IDENT_* words."""
    params: np.ndarray
    cost0: np.ndarray
    cost: np.ndarray
    evals: np.ndarray
    status: np.ndarray
    wind: Optional[np.ndarray] = None      # identify_joint: (B, 3) the identified wind offset w


class BatchNMPC:
    """A batch of independent NMPC instances on one GPU (one C-ABI context)."""

    def __init__(self, params: Optional[KiteParams] = None, config: Optional[NmpcConfig] = None,
                 batch: int = 1):
        self.params = params if params is not None else load_properties()
        self.config = config if config is not None else default_config()
        self.batch = int(batch)
        self.N = int(self.config.N)
        h = ctypes.c_void_p()
        _check(lib().kite_nmpc_create(ctypes.byref(self.params), ctypes.byref(self.config), self.batch,
                                      ctypes.byref(h)), "kite_nmpc_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().kite_nmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # --- configuration ----------------------------------------------------
    def set_bounds(self, lbx=None, ubx=None, lbu=None, ubu=None):
        args = [None if a is None else _f64(a) for a in (lbx, ubx, lbu, ubu)]
        _check(lib().kite_nmpc_set_bounds(self._h, *[_p(a) for a in args]), "set_bounds")

    def set_reference_velocity(self, v: float):
        _check(lib().kite_nmpc_set_reference_velocity(self._h, float(v)), "set_reference_velocity")

    def reset(self):
        _check(lib().kite_nmpc_reset(self._h), "reset")

    def set_wind(self, wind=None):
        """Per-kite constant world-frame wind, (B, 3) m/s, for wind-field sweeps
        (kite_nmpc_set_wind; None or all zero = the reference model, which has
        no wind)."""
        if wind is None:
            _check(lib().kite_nmpc_set_wind(self._h, None), "set_wind")
            return
        w = np.ascontiguousarray(np.asarray(wind, dtype=np.float64).reshape(self.batch, 3))
        _check(lib().kite_nmpc_set_wind(self._h, w.ctypes.data_as(_DP)), "set_wind")

    def set_stream(self, stream_ptr: int):
        """Run on this hipStream_t (int handle; 0 = the HIP null stream, which is
        torch's default stream)."""
        _check(lib().kite_nmpc_set_stream(self._h, ctypes.c_void_p(stream_ptr) if stream_ptr else None),
               "set_stream")

    def use_own_stream(self):
        _check(lib().kite_nmpc_use_own_stream(self._h), "use_own_stream")

    def synchronize(self):
        _check(lib().kite_nmpc_synchronize(self._h), "synchronize")

    # --- RTI step -------------------------------------------------------------
    def step(self, x0: np.ndarray, want_traj: bool = True):
        B, N = self.batch, self.N
        x0 = _f64(x0).reshape(B, 15)
        u0 = np.zeros((B, 4))
        traj = np.zeros((B, N + 1, 15)) if want_traj else None
        ctrl = np.zeros((B, N, 4)) if want_traj else None
        diag = (MpcDiagnostic * B)()
        status = np.zeros(B, dtype=np.int32)
        _check(lib().kite_nmpc_step(self._h, _p(x0), _p(u0), _p(traj), _p(ctrl), diag,
                                    status.ctypes.data_as(_IP)), "kite_nmpc_step")
        d = np.ctypeslib.as_array(ctypes.cast(diag, _DP), shape=(B, 6)).copy()
        return dict(u0=u0, traj=traj, ctrl=ctrl, diag=d, status=status)

    def step_device(self, x0_ptr: int, u0_ptr=0, traj_ptr=0, ctrl_ptr=0, diag_ptr=0, status_ptr=0):
        v = lambda p: ctypes.c_void_p(p) if p else None
        _check(lib().kite_nmpc_step_device(self._h, v(x0_ptr), v(u0_ptr), v(traj_ptr), v(ctrl_ptr),
                                           v(diag_ptr), v(status_ptr)), "kite_nmpc_step_device")

    def get_solution(self):
        traj = np.zeros((self.batch, self.N + 1, 15)); ctrl = np.zeros((self.batch, self.N, 4))
        _check(lib().kite_nmpc_get_solution(self._h, _p(traj), _p(ctrl)), "get_solution")
        return traj, ctrl

    def set_solution(self, traj, ctrl):
        _check(lib().kite_nmpc_set_solution(self._h, _p(_f64(traj)), _p(_f64(ctrl))), "set_solution")

    TIMING_KEYS = ("prologue", "rk4_sens", "condense", "qp", "total", "qp_main")

    def kernel_times(self):
        """Device time [ms] of the last step per phase (config.timing = 1);
        qp is the QP phase (solve + expansion + lazy rows), qp_main the main
        QP kernel alone."""
        ms = np.zeros(6)
        n = _check(lib().kite_nmpc_kernel_times(self._h, _p(ms), 6), "kernel_times")
        return dict(zip(self.TIMING_KEYS, ms[:n]))

    def timing_start(self, max_steps: int, stride: int = 1):
        """Record the kernel events of every stride-th step from the next one
        on, at most max_steps of them (kite_nmpc_timing_start_sampled)."""
        if stride == 1:
            _check(lib().kite_nmpc_timing_start(self._h, int(max_steps)), "timing_start")
        else:
            _check(lib().kite_nmpc_timing_start_sampled(self._h, int(max_steps), int(stride)), "timing_start")

    def timing_read(self):
        """Per-phase SUMS [ms] over the steps recorded since timing_start
        (keys as kernel_times)."""
        ms = np.zeros(6)
        n = _check(lib().kite_nmpc_timing_read(self._h, _p(ms), 6), "timing_read")
        return n, dict(zip(self.TIMING_KEYS, ms))

    def qp_stats(self):
        kkt = np.zeros(self.batch); it = np.zeros(self.batch, dtype=np.int32)
        _check(lib().kite_nmpc_qp_stats(self._h, _p(kkt), it.ctypes.data_as(_IP)), "qp_stats")
        return kkt, it

    def qp_iteration_sum(self) -> int:
        """QP iterations summed over instances and steps since timing_start."""
        v = ctypes.c_int64(0)
        _check(lib().kite_nmpc_qp_iteration_sum(self._h, ctypes.byref(v)), "qp_iteration_sum")
        return int(v.value)

    def state_bound_stats(self):
        """(kite-steps outside the state box, (node, state) pairs outside it),
        summed over instances and steps since timing_start (status bit 8 and
        the violated state rows of the committed plans)."""
        a, r = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(lib().kite_nmpc_state_bound_stats(self._h, ctypes.byref(a), ctypes.byref(r)), "state_bound_stats")
        return int(a.value), int(r.value)

    def get_qp(self, instance: int):
        n = 4 * self.N + 2
        H = np.zeros((n, n)); h = np.zeros(n); C = np.zeros((self.N, n)); cl = np.zeros(self.N); cu = np.zeros(self.N)
        _check(lib().kite_nmpc_get_qp(self._h, int(instance), _p(H), _p(h), _p(C), _p(cl), _p(cu)), "get_qp")
        return dict(H=H, h=h, C=C, cl=cl, cu=cu)

    # --- model-level ----------------------------------------------------------
    def closest_point(self, pos, guess=None):
        pos = _f64(pos).reshape(-1, 3)
        out = np.zeros(pos.shape[0])
        g = None if guess is None else _f64(guess).reshape(-1)
        _check(lib().kite_nmpc_closest_point(self._h, pos.shape[0], _p(pos), _p(g), _p(out)), "closest_point")
        return out

    # --- closed-loop scoring ----------------------------------------------------
    def closest_point_global(self, pos):
        """The global closest point of the path to every position (count, 3):
        (theta* in [-2 pi / 64, 2 pi), d = ||P(theta*) - pos||), NaN for a
        non-finite position (kite_nmpc_closest_point_global)."""
        pos = _f64(pos).reshape(-1, 3)
        th = np.zeros(pos.shape[0]); d = np.zeros(pos.shape[0])
        _check(lib().kite_nmpc_closest_point_global(self._h, pos.shape[0], _p(pos), _p(th), _p(d)),
               "closest_point_global")
        return th, d

    def closest_point_global_device(self, count: int, d_pos3: int, d_theta: int, d_dist: int):
        _check(lib().kite_nmpc_closest_point_global_device(self._h, int(count), d_pos3, d_theta, d_dist),
               "closest_point_global_device")

    def score_step(self, x13, u4, acc, mem, status=None, plant_status=None, first: bool = False):
        """One control period of every kite into acc (count, 16) and mem
        (count, 8), both updated in place and returned (kite_nmpc_score_step;
        the slots are SCORE_*).  status / plant_status: (count,) int32 words."""
        x = _f64(x13).reshape(-1, 13); u = _f64(u4).reshape(-1, 4)
        c = x.shape[0]
        assert u.shape[0] == c and acc.shape == (c, SCORE_NACC) and mem.shape == (c, SCORE_NMEM)
        st = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(c)
        ps = None if plant_status is None else np.ascontiguousarray(plant_status, dtype=np.int32).reshape(c)
        _check(lib().kite_nmpc_score_step(self._h, c, _p(x), _p(u), st.ctypes.data_as(_IP) if st is not None else None,
                                          ps.ctypes.data_as(_IP) if ps is not None else None, int(bool(first)),
                                          _p(acc), _p(mem)), "score_step")
        return acc, mem

    def score_step_device(self, count: int, d_x13: int, d_u4: int, d_status: int, d_plant_status: int, first: bool,
                          d_acc: int, d_mem: int):
        """Device pointers, asynchronous on the context's stream (0: no status word)."""
        _check(lib().kite_nmpc_score_step_device(self._h, int(count), d_x13, d_u4, d_status or None,
                                                 d_plant_status or None, int(bool(first)), d_acc, d_mem),
               "score_step_device")

    def score_summary(self, acc):
        """The raw fleet summary (16,) of acc (count, 16) (kite_nmpc_score_summary);
        ``score_derive`` makes the readable figures from it."""
        a = _f64(acc).reshape(-1, SCORE_NACC)
        out = np.zeros(SCORE_NSUM)
        _check(lib().kite_nmpc_score_summary(self._h, a.shape[0], _p(a), _p(out)), "score_summary")
        return out

    def score_summary_device(self, count: int, d_acc: int, d_out16: int):
        _check(lib().kite_nmpc_score_summary_device(self._h, int(count), d_acc, d_out16), "score_summary_device")

    def dynamics(self, x15, u4):
        x = _f64(x15).reshape(-1, 15); u = _f64(u4).reshape(-1, 4)
        f = np.zeros_like(x)
        _check(lib().kite_nmpc_dynamics(self._h, x.shape[0], _p(x), _p(u), _p(f)), "dynamics")
        return f

    def jacobian(self, x13, u3):
        x = _f64(x13).reshape(-1, 13); u = _f64(u3).reshape(-1, 3)
        Jx = np.zeros((x.shape[0], 13, 13)); Ju = np.zeros((x.shape[0], 13, 3))
        _check(lib().kite_nmpc_jacobian(self._h, x.shape[0], _p(x), _p(u), _p(Jx), _p(Ju)), "jacobian")
        return Jx, Ju

    def colloc_eval(self, cfg: "CollocConfig", z, jac: bool = False):
        """Reference collocation residual G (count x n*15), cost J (count) and,
        with jac, the per-node blocks d SODE / d [x, u] (count x n x 15 x 19)."""
        n = cfg.poly_order * cfg.num_segments + 1
        zz = _f64(z).reshape(-1, n * 19)
        c = zz.shape[0]
        G = np.zeros((c, n * 15)); J = np.zeros(c)
        Jb = np.zeros((c, n, 15, 19)) if jac else None
        _check(lib().kite_nmpc_colloc_eval(self._h, ctypes.byref(cfg), c, _p(zz), _p(G), _p(J), _p(Jb)), "colloc_eval")
        return (G, J, Jb) if jac else (G, J)

    def ekf_step_device(self, count: int, dt: float, d_x13: int, d_u3: int, d_P169: int, d_z7: int,
                        d_W169: int, d_V49: int):
        """Device-pointer EKF step (asynchronous on the context stream)."""
        _check(lib().kite_nmpc_ekf_step_device(self._h, int(count), float(dt), d_x13, d_u3, d_P169, d_z7 or None,
                                               d_W169, d_V49), "ekf_step_device")

    def ekf_step(self, x13, u3, P, dt: float, z7=None, W=None, V=None):
        """Batched KiteEKF propagate (+ update when z7 is given); returns (x, P)."""
        x = _f64(x13).reshape(-1, 13).copy()
        c = x.shape[0]
        Pm = _f64(P).reshape(c, 13, 13).copy()
        u = _f64(u3).reshape(c, 3)
        Wd, Vd, _ = ekf_default_covariances()
        W = Wd if W is None else _f64(W).reshape(13, 13)
        V = Vd if V is None else _f64(V).reshape(7, 7)
        z = None if z7 is None else _f64(z7).reshape(c, 7)
        _check(lib().kite_nmpc_ekf_step(self._h, c, float(dt), _p(x), _p(u), _p(Pm), _p(z), _p(W), _p(V)),
               "ekf_step")
        return x, Pm

    def wind_ekf_step_device(self, count: int, dt: float, substeps: int, d_x16: int, d_u3: int, d_P256: int,
                             d_z7: int, d_W256: int, d_V49: int, d_status: int = 0):
        """Device-pointer step of the wind-estimating EKF (asynchronous on the
        context stream): `substeps` propagations of dt / substeps and, with
        d_z7, one update; d_status (count int32) receives the KITE_EKF_* words."""
        _check(lib().kite_nmpc_windekf_step_device(self._h, int(count), float(dt), int(substeps), d_x16, d_u3, d_P256,
                                                   d_z7 or None, d_W256, d_V49 or None, d_status or None),
               "wind_ekf_step_device")

    def wind_ekf_step(self, x16, u3, P, dt: float, substeps: int = 1, z7=None, W=None, V=None):
        """Batched wind-estimating EKF (kite_nmpc_windekf_step): the state is
        [x13 | W3], P (count, 16, 16); `substeps` propagations of dt / substeps
        under the estimated wind, then one update when z7 is given.  Returns
        (x16, P, status), status the KITE_EKF_* words (``EKF_NAN``,
        ``EKF_S_NOT_PD``)."""
        x = _f64(x16).reshape(-1, 16).copy()
        c = x.shape[0]
        Pm = _f64(P).reshape(c, 16, 16).copy()
        u = _f64(u3).reshape(c, 3)
        Wd, Vd, _ = wind_ekf_default_covariances()
        W = Wd if W is None else _f64(W).reshape(16, 16)
        V = Vd if V is None else _f64(V).reshape(7, 7)
        z = None if z7 is None else _f64(z7).reshape(c, 7)
        st = np.zeros(c, dtype=np.int32)
        _check(lib().kite_nmpc_windekf_step(self._h, c, float(dt), int(substeps), _p(x), _p(u), _p(Pm), _p(z), _p(W),
                                            _p(V), st.ctypes.data_as(_IP)), "wind_ekf_step")
        return x, Pm, st

    def jacobian_wind(self, x13, u3, w3):
        """[df/dx | df/dW] (count, 13, 16) of the wind model at (x13, u3) under
        the winds w3 (count, 3): the wind-estimating filter's Jacobian pass."""
        x = _f64(x13).reshape(-1, 13); u = _f64(u3).reshape(-1, 3); w = _f64(w3).reshape(-1, 3)
        J = np.zeros((x.shape[0], 13, 16))
        _check(lib().kite_nmpc_jacobian_wind(self._h, x.shape[0], _p(x), _p(u), _p(w), _p(J)), "jacobian_wind")
        return J

    def set_wind_device(self, ptr: int, stride: int = 3, wmax: float = WIND_MAX_DEFAULT):
        """``set_wind`` from device memory (kite_nmpc_set_wind_device,
        asynchronous on the context stream): B winds `stride` doubles apart at
        ptr, each component clamped to +-wmax, a non-finite one replaced by 0."""
        _check(lib().kite_nmpc_set_wind_device(self._h, ctypes.c_void_p(ptr) if ptr else None, int(stride),
                                               float(wmax)), "set_wind_device")

    # --- kinematic (pose-only) EKF ----------------------------------------------
    def kin_ekf_step_device(self, count: int, dt: float, substeps: int, d_x13: int, d_P169: int, d_z7: int,
                            d_W169: int, d_V49: int, d_status: int = 0, frame=None):
        """Device-pointer step of the kinematic EKF (kite_nmpc_kinekf_step_device,
        asynchronous on the context stream); frame: a ``PoseFrame`` on the
        host, passed by value into the launch, or None."""
        _check(lib().kite_nmpc_kinekf_step_device(self._h, int(count), float(dt), int(substeps), d_x13, d_P169,
                                                  d_z7 or None, d_W169, d_V49 or None, _frame(frame),
                                                  d_status or None), "kin_ekf_step_device")

    def kin_ekf_step(self, x13, P, dt: float, substeps: int = 1, z7=None, W=None, V=None, frame=None):
        """Batched kinematic EKF (kite_nmpc_kinekf_step): the model-free filter
        of the reference's estimator node, P (count, 13, 13); `substeps`
        propagations of dt / substeps, then one update when z7 is given.  frame
        (a ``PoseFrame``): z7 are motion-capture poses and are moved to the world
        frame first, on a copy; None: world poses.  Returns (x13, P, status),
        status the KITE_EKF_* words (``EKF_NAN``, ``EKF_S_NOT_PD``)."""
        x = _f64(x13).reshape(-1, 13).copy()
        c = x.shape[0]
        Pm = _f64(P).reshape(c, 13, 13).copy()
        Wd, Vd, _ = ekf_default_covariances()
        W = Wd if W is None else _f64(W).reshape(13, 13)
        V = Vd if V is None else _f64(V).reshape(7, 7)
        z = None if z7 is None else _f64(z7).reshape(c, 7)
        st = np.zeros(c, dtype=np.int32)
        _check(lib().kite_nmpc_kinekf_step(self._h, c, float(dt), int(substeps), _p(x), _p(Pm), _p(z), _p(W), _p(V),
                                           _frame(frame), st.ctypes.data_as(_IP)), "kin_ekf_step")
        return x, Pm, st

    def kin_ekf_init_device(self, count: int, dt: float, d_prev7: int, d_new7: int, d_x13: int, d_status: int = 0,
                            frame=None):
        """Device-pointer form of ``kin_ekf_init`` (asynchronous on the context stream)."""
        _check(lib().kite_nmpc_kinekf_init_device(self._h, int(count), float(dt), d_prev7, d_new7, _frame(frame),
                                                  d_x13, d_status or None), "kin_ekf_init_device")

    def kin_ekf_init(self, pose_prev, pose_new, dt: float, frame=None, x13=None):
        """The 13 states from two consecutive poses (count, 7) dt apart
        (kite_nmpc_kinekf_init: KiteEKF_Node::initialize).  Returns (x13,
        status); a kite with ``EKF_INIT_BAD`` (dt <= 0 or non-finite, a
        non-finite pose) keeps its row of the x13 passed in (zeros without)."""
        mp = _f64(pose_prev).reshape(-1, 7); mn = _f64(pose_new).reshape(-1, 7)
        c = mp.shape[0]
        if mn.shape[0] != c:
            raise ValueError("pose_prev and pose_new: one pose per kite each")
        x = np.zeros((c, 13)) if x13 is None else _f64(x13).reshape(c, 13).copy()
        st = np.zeros(c, dtype=np.int32)
        _check(lib().kite_nmpc_kinekf_init(self._h, c, float(dt), _p(mp), _p(mn), _frame(frame), _p(x),
                                           st.ctypes.data_as(_IP)), "kin_ekf_init")
        return x, st

    def jacobian_kin(self, x13):
        """df/dx (count, 13, 13) of the kinematic model at x13: the kinematic
        filter's Jacobian pass."""
        x = _f64(x13).reshape(-1, 13)
        J = np.zeros((x.shape[0], 13, 13))
        _check(lib().kite_nmpc_jacobian_kin(self._h, x.shape[0], _p(x), _p(J)), "jacobian_kin")
        return J

    @staticmethod
    def pose_frame_default() -> PoseFrame:
        """The reference node's frame (kite_pose_frame_default)."""
        return pose_frame_default()

    # --- per-kite controller models --------------------------------------------
    def set_params(self, rows=None):
        """The model of the step's predictions (kite_nmpc_set_params): None =
        the creation model, one ``KiteParams`` (or 52 values) = one model for
        every kite, a (B, 52) array = a model per kite (see ``perturb_params``).
        The item-wise entry points and the plant's default keep the creation
        model; so do the EKFs unless ``set_estimator_model`` says otherwise."""
        if rows is None:
            _check(lib().kite_nmpc_set_params(self._h, None, 0), "set_params")
            return
        if isinstance(rows, KiteParams):
            rows = rows.as_array()
        p = _f64(rows)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        if p.ndim != 2 or p.shape[1] != len(_PARAM_FIELDS):
            raise ValueError("controller parameters: 52 values per kite")
        _check(lib().kite_nmpc_set_params(self._h, ctypes.c_void_p(p.ctypes.data), p.shape[0]), "set_params")

    def set_params_device(self, ptr: int, count: int, status_ptr: int = 0):
        """``set_params`` with a row per kite from device memory
        (kite_nmpc_set_params_device, asynchronous on the context stream): count
        = B rows of 52 doubles at ptr.  A row that is no model keeps that kite's
        previous one and sets ``PARAMS_REJECTED`` in the int32 status word at
        status_ptr (B words, optional)."""
        v = lambda p: ctypes.c_void_p(p) if p else None
        _check(lib().kite_nmpc_set_params_device(self._h, v(ptr), int(count), v(status_ptr)), "set_params_device")

    def get_params(self) -> np.ndarray:
        """The (B, 52) rows in force (kite_nmpc_get_params)."""
        out = np.zeros((self.batch, len(_PARAM_FIELDS)))
        _check(lib().kite_nmpc_get_params(self._h, ctypes.c_void_p(out.ctypes.data)), "get_params")
        return out

    def set_estimator_model(self, mode: int):
        """The model of ``ekf_step`` / ``wind_ekf_step`` and their device forms
        (not of ``kin_ekf_step``, which has no model)
        (kite_nmpc_set_estimator_model): ``EST_MODEL_CREATION`` (the default) or
        ``EST_MODEL_CONTROLLER``, the controller's models in force at each call
        (``set_params[_device]``).  With a model per kite in force kite b
        filters with row b and a call's count must be the batch."""
        _check(lib().kite_nmpc_set_estimator_model(self._h, int(mode)), "set_estimator_model")

    def set_qp_split(self, mode: int):
        """The two-phase tiled QP at N = 20 (kite_nmpc_set_qp_split):
        ``QP_SPLIT_AUTO`` (the default: split where several QP waves queue per
        SIMD), ``QP_SPLIT_NEVER`` (one launch) or any positive value (split at
        any batch).  The results are bitwise the same in every mode."""
        _check(lib().kite_nmpc_set_qp_split(self._h, int(mode)), "set_qp_split")

    def qp_split(self) -> dict:
        """``mode`` set, whether the next step splits (``active``), the build's
        ``split_iteration`` and the ``split_launches`` issued so far (a step
        replayed from a captured graph counts once, at its capture)."""
        m, a, k = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        n = ctypes.c_int64(0)
        _check(lib().kite_nmpc_get_qp_split(self._h, ctypes.byref(m), ctypes.byref(a), ctypes.byref(k),
                                            ctypes.byref(n)), "get_qp_split")
        return dict(mode=int(m.value), active=bool(a.value), split_iteration=int(k.value),
                    split_launches=int(n.value))

    @property
    def estimator_model(self) -> int:
        m = ctypes.c_int32(0)
        _check(lib().kite_nmpc_get_estimator_model(self._h, ctypes.byref(m)), "get_estimator_model")
        return int(m.value)

    def predict(self, x15, u4, tf: float, steps: int = 1):
        x = _f64(x15).reshape(-1, 15); u = _f64(u4).reshape(-1, 4)
        xo = np.zeros_like(x)
        _check(lib().kite_nmpc_predict(self._h, x.shape[0], _p(x), _p(u), float(tf), int(steps), _p(xo)), "predict")
        return xo

    # --- plant simulator --------------------------------------------------------
    def plant_set_params(self, params=None):
        """The plant's model (kite_nmpc_plant_set_params): None = the
        controller's own parameters, one ``KiteParams`` (or 52 values) = one
        plant model for every kite, a (B, 52) array = a model per kite (see
        ``perturb_params``)."""
        if params is None:
            _check(lib().kite_nmpc_plant_set_params(self._h, None, 0), "plant_set_params")
            return
        if isinstance(params, KiteParams):
            params = params.as_array()
        p = _f64(params)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        if p.ndim != 2 or p.shape[1] != len(_PARAM_FIELDS):
            raise ValueError("plant parameters: 52 values per kite")
        _check(lib().kite_nmpc_plant_set_params(self._h, ctypes.c_void_p(p.ctypes.data), p.shape[0]),
               "plant_set_params")

    def plant_set_wind(self, wind=None, gust_amp=None, gust_hz=None, gust_phase=None):
        """The wind the plant sees (kite_nmpc_plant_set_wind), world frame, m/s:
        W(t) = wind + gust_amp sin(2 pi gust_hz t + gust_phase) per kite.  wind
        and gust_amp are (B, 3) or (3,), gust_hz and gust_phase (B,) or scalars;
        omitted parts are zero, all omitted = no wind.  The controller's model
        is not told (that is ``set_wind``)."""
        if wind is None and gust_amp is None and gust_hz is None and gust_phase is None:
            _check(lib().kite_nmpc_plant_set_wind(self._h, None), "plant_set_wind")
            return
        B = self.batch
        w8 = np.zeros((B, 8))
        if wind is not None:
            w8[:, 0:3] = np.broadcast_to(np.asarray(wind, dtype=np.float64), (B, 3))
        if gust_amp is not None:
            w8[:, 3:6] = np.broadcast_to(np.asarray(gust_amp, dtype=np.float64), (B, 3))
        if gust_hz is not None:
            w8[:, 6] = np.broadcast_to(np.asarray(gust_hz, dtype=np.float64), (B,))
        if gust_phase is not None:
            w8[:, 7] = np.broadcast_to(np.asarray(gust_phase, dtype=np.float64), (B,))
        _check(lib().kite_nmpc_plant_set_wind(self._h, _p(w8)), "plant_set_wind")

    def plant_step(self, x13, u4, t0: float, h: float, steps: int = 1, substeps: int = 4):
        """Advance the (B, 13) plant states from t0 over steps * h under the held
        control u4 (B, 4), RK4 with `substeps` per step; returns (x13, status),
        status the KITE_PLANT_* words (``PLANT_NAN``)."""
        x = _f64(x13).reshape(self.batch, 13).copy()
        u = _f64(u4).reshape(self.batch, 4)
        st = np.zeros(self.batch, dtype=np.int32)
        _check(lib().kite_nmpc_plant_step(self._h, _p(x), _p(u), float(t0), float(h), int(steps), int(substeps),
                                          st.ctypes.data_as(_IP)), "plant_step")
        return x, st

    def plant_step_device(self, x13_ptr: int, u4_ptr: int, t0: float, h: float, steps: int = 1, substeps: int = 4,
                          status_ptr: int = 0):
        """plant_step in place on device pointers (asynchronous on the context stream)."""
        v = lambda p: ctypes.c_void_p(p) if p else None
        _check(lib().kite_nmpc_plant_step_device(self._h, v(x13_ptr), v(u4_ptr), float(t0), float(h), int(steps),
                                                 int(substeps), v(status_ptr)), "plant_step_device")

    def plant_step_delayed(self, x13, u4_cmd, tau, line, t0: float, h: float, steps: int = 1, substeps: int = 4):
        """One control period of the plant behind the per-kite command line
        (kite_nmpc_plant_step_delayed): u4_cmd (B, 4), or None to send nothing,
        is sent at t0 with the latencies tau (B,); the commands that have
        arrived take effect at the plant ticks.  line: (B, DELAY_NLINE), all
        zero = a fresh line.  Returns (x13, line, u_applied, status): the new
        state and line, the control in force during the last plant step and
        the KITE_PLANT_* words (``PLANT_NAN``, ``PLANT_CMD_DROPPED``,
        ``PLANT_BAD_TAU``)."""
        B = self.batch
        x, ln = _f64(x13), _f64(line)
        if x.shape != (B, 13):
            raise ValueError(f"x13: ({B}, 13) expected, got {x.shape}")
        if ln.shape != (B, DELAY_NLINE):
            raise ValueError(f"line: ({B}, {DELAY_NLINE}) expected, got {ln.shape}")
        u = ta = None
        if u4_cmd is not None:
            u = _f64(u4_cmd)
            if u.shape != (B, 4):
                raise ValueError(f"u4_cmd: ({B}, 4) expected, got {u.shape}")
            if tau is None:
                raise ValueError("a command needs its latency: tau (B,)")
            ta = _f64(tau)
            if ta.shape != (B,):
                raise ValueError(f"tau: ({B},) expected, got {ta.shape}")
        x, ln = x.copy(), ln.copy()
        ua = np.zeros((B, 4))
        st = np.zeros(B, dtype=np.int32)
        _check(lib().kite_nmpc_plant_step_delayed(self._h, _p(x), _p(u), _p(ta), _p(ln), _p(ua), float(t0), float(h),
                                                  int(steps), int(substeps), st.ctypes.data_as(_IP)),
               "plant_step_delayed")
        return x, ln, ua, st

    def plant_step_delayed_device(self, x13_ptr: int, u4_cmd_ptr: int, tau_ptr: int, line_ptr: int, t0: float,
                                  h: float, steps: int = 1, substeps: int = 4, u4_applied_ptr: int = 0,
                                  status_ptr: int = 0):
        """plant_step_delayed in place on device pointers (asynchronous on the
        context stream); u4_cmd_ptr 0: nothing is sent."""
        v = lambda p: ctypes.c_void_p(p) if p else None
        _check(lib().kite_nmpc_plant_step_delayed_device(self._h, v(x13_ptr), v(u4_cmd_ptr), v(tau_ptr), v(line_ptr),
                                                         v(u4_applied_ptr), float(t0), float(h), int(steps),
                                                         int(substeps), v(status_ptr)), "plant_step_delayed_device")

    # --- the in-flight schedule of the delay compensation ----------------------
    def set_inflight(self, line, t0: float = 0.0):
        """The commands in flight as the delay compensation sees them
        (kite_nmpc_set_inflight): line (B, DELAY_NLINE), the kites' command
        lines as they stand at time t0, becomes the context's schedule; warm
        steps with config.delay > 0 then predict under the control in force
        and the pending commands instead of the previous u(t0).  None switches
        the schedule off.  It stays in force as stored: refresh it every
        period, right before the step."""
        if line is None:
            _check(lib().kite_nmpc_set_inflight(self._h, None, float(t0)), "set_inflight")
            return
        ln = _f64(line)
        if ln.shape != (self.batch, DELAY_NLINE):
            raise ValueError(f"line: ({self.batch}, {DELAY_NLINE}) expected, got {ln.shape}")
        _check(lib().kite_nmpc_set_inflight(self._h, _p(ln), float(t0)), "set_inflight")

    def set_inflight_device(self, line_ptr: int, t0: float = 0.0):
        """set_inflight from a (B, DELAY_NLINE) device array (asynchronous on the
        context stream, the line is read in stream order); 0 switches it off."""
        _check(lib().kite_nmpc_set_inflight_device(self._h, ctypes.c_void_p(line_ptr) if line_ptr else None,
                                                   float(t0)), "set_inflight_device")

    def get_inflight(self) -> np.ndarray:
        """The schedule rows in force, (B, INFLIGHT_N): [n | s_1..s_4 | control in
        force (3) | pending commands (4 x 3) | zeros]; n = -1 marks an invalid row."""
        out = np.zeros((self.batch, INFLIGHT_N))
        _check(lib().kite_nmpc_get_inflight(self._h, _p(out)), "get_inflight")
        return out

    # --- aerodynamic parameter identification ---------------------------------
    def _ident_rows(self, params, count: int) -> np.ndarray:
        """(1, 52) or (count, 52) rows of kite_params; None: the context's own."""
        if params is None:
            params = self.params
        if isinstance(params, KiteParams):
            params = params.as_array()
        p = _f64(params)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        if p.ndim != 2 or p.shape[1] != len(_PARAM_FIELDS) or p.shape[0] not in (1, count):
            raise ValueError("identification parameters: 52 values, one row or one per kite")
        return p

    @staticmethod
    def _ident_wind(wind, B: int, T: Optional[int]) -> np.ndarray:
        """The wind of the identification as a contiguous array: (B, 3) for
        ``ident_sens`` (T None), else the log (B, T, 3); there a (B, 3) array is
        one wind per kite, held over its T samples."""
        w = _f64(wind)
        if T is None:
            if w.shape != (B, 3):
                raise ValueError(f"wind: (count, 3) = ({B}, 3), got {w.shape}")
            return w
        if w.shape == (B, 3):
            w = np.ascontiguousarray(np.broadcast_to(w[:, None, :], (B, T, 3)))
        if w.shape != (B, T, 3):
            raise ValueError(f"wind: (B, T, 3) = ({B}, {T}, 3) or (B, 3), got {w.shape}")
        return w

    def ident_sens(self, x13, u3, h: float, substeps: int = 4, params=None, wind=None):
        """One sample interval per item (kite_nmpc_ident_sens): x+ (count, 13) and
        S = d x+ / d p (count, 13, 21, unscaled) with respect to ``IDENT_FIELDS``.
        wind (count, 3): the item's world-frame wind (kite_nmpc_ident_sens_wind);
        None: the windless model."""
        x = _f64(x13).reshape(-1, 13); u = _f64(u3).reshape(-1, 3)
        c = x.shape[0]
        p = self._ident_rows(params, c)
        xo = np.zeros((c, 13)); S = np.zeros((c, 13, IDENT_NP))
        if wind is not None:
            w = self._ident_wind(wind, c, None)
            _check(lib().kite_nmpc_ident_sens_wind(self._h, c, float(h), int(substeps),
                                                   ctypes.c_void_p(p.ctypes.data), p.shape[0], _p(x), _p(u), _p(w),
                                                   _p(xo), _p(S)), "ident_sens_wind")
            return xo, S
        _check(lib().kite_nmpc_ident_sens(self._h, c, float(h), int(substeps), ctypes.c_void_p(p.ctypes.data),
                                          p.shape[0], _p(x), _p(u), _p(xo), _p(S)), "ident_sens")
        return xo, S

    def ident_normal(self, X, U, p21, params=None, config: Optional[IdentConfig] = None, wind=None):
        """One evaluation of the identification's normal equations at the
        parameter values p21 (B, 21) on the logs X (B, T+1, 13), U (B, T, 3):
        (A (B, 21, 21), g (B, 21), cost (B,), status (B,)) in the scaled variables.
        wind: the logged world-frame wind (B, T, 3), or (B, 3) held over the log
        (kite_nmpc_ident_normal_wind); None: the windless model."""
        cfg = config if config is not None else ident_default_config()
        X = _f64(X); U = _f64(U)
        B, T = U.shape[0], U.shape[1]
        if X.shape != (B, T + 1, 13) or U.shape != (B, T, 3):
            raise ValueError("logs: X (B, T+1, 13), U (B, T, 3)")
        p = self._ident_rows(params, B)
        q = _f64(p21).reshape(B, IDENT_NP)
        A = np.zeros((B, IDENT_NP, IDENT_NP)); g = np.zeros((B, IDENT_NP)); cost = np.zeros(B)
        st = np.zeros(B, dtype=np.int32)
        if wind is not None:
            w = self._ident_wind(wind, B, T)
            _check(lib().kite_nmpc_ident_normal_wind(self._h, ctypes.byref(cfg), B, T, ctypes.c_void_p(p.ctypes.data),
                                                     p.shape[0], _p(q), _p(X), _p(U), _p(w), _p(A), _p(g), _p(cost),
                                                     st.ctypes.data_as(_IP)), "ident_normal_wind")
            return A, g, cost, st
        _check(lib().kite_nmpc_ident_normal(self._h, ctypes.byref(cfg), B, T, ctypes.c_void_p(p.ctypes.data),
                                            p.shape[0], _p(q), _p(X), _p(U), _p(A), _p(g), _p(cost),
                                            st.ctypes.data_as(_IP)), "ident_normal")
        return A, g, cost, st

    def identify(self, X, U, params=None, config: Optional[IdentConfig] = None, wind=None) -> IdentResult:
        """Fit the 21 aerodynamic coefficients (``IDENT_FIELDS``) of every kite to
        its log X (B, T+1, 13), U (B, T, 3) (kite_nmpc_identify).  params: the
        kites' rows (52 values, one for all or (B, 52)), whose 21 are the start
        and the centre of the box; None: the context's own.  wind: the known
        world-frame wind the log was flown under, (B, T, 3) with row k held over
        sample interval k, or (B, 3) held over the log (kite_nmpc_identify_wind);
        None: the windless model."""
        cfg = config if config is not None else ident_default_config()
        X = _f64(X); U = _f64(U)
        B, T = U.shape[0], U.shape[1]
        if X.shape != (B, T + 1, 13) or U.shape != (B, T, 3):
            raise ValueError("logs: X (B, T+1, 13), U (B, T, 3)")
        p = self._ident_rows(params, B)
        out = np.zeros((B, len(_PARAM_FIELDS))); c2 = np.zeros((B, 2))
        ev = np.zeros(B, dtype=np.int32); st = np.zeros(B, dtype=np.int32)
        if wind is not None:
            w = self._ident_wind(wind, B, T)
            _check(lib().kite_nmpc_identify_wind(self._h, ctypes.byref(cfg), B, T, ctypes.c_void_p(p.ctypes.data),
                                                 p.shape[0], _p(X), _p(U), _p(w), ctypes.c_void_p(out.ctypes.data),
                                                 _p(c2), ev.ctypes.data_as(_IP), st.ctypes.data_as(_IP)),
                   "identify_wind")
            return IdentResult(out, c2[:, 0].copy(), c2[:, 1].copy(), ev, st)
        _check(lib().kite_nmpc_identify(self._h, ctypes.byref(cfg), B, T, ctypes.c_void_p(p.ctypes.data), p.shape[0],
                                        _p(X), _p(U), ctypes.c_void_p(out.ctypes.data), _p(c2),
                                        ev.ctypes.data_as(_IP), st.ctypes.data_as(_IP)), "identify")
        return IdentResult(out, c2[:, 0].copy(), c2[:, 1].copy(), ev, st)

    def identify_device(self, config: IdentConfig, count: int, T: int, params_ptr: int, nparams: int, X_ptr: int,
                        U_ptr: int, params_out_ptr: int, cost2_ptr: int = 0, evals_ptr: int = 0, status_ptr: int = 0,
                        workspace_ptr: int = 0, wind: int = 0):
        """identify on device pointers (kite_nmpc_identify_device): 2 * iters
        launches on the context stream, nothing allocated, copied or awaited;
        the workspace holds ``ident_workspace_doubles`` doubles.  wind: device
        pointer of the wind log (count, T, 3) (kite_nmpc_identify_wind_device);
        0: the windless model."""
        v = lambda p: ctypes.c_void_p(p) if p else None
        if wind:
            _check(lib().kite_nmpc_identify_wind_device(self._h, ctypes.byref(config), int(count), int(T),
                                                        v(params_ptr), int(nparams), v(X_ptr), v(U_ptr), v(wind),
                                                        v(params_out_ptr), v(cost2_ptr), v(evals_ptr), v(status_ptr),
                                                        v(workspace_ptr)), "identify_wind_device")
            return
        _check(lib().kite_nmpc_identify_device(self._h, ctypes.byref(config), int(count), int(T), v(params_ptr),
                                               int(nparams), v(X_ptr), v(U_ptr), v(params_out_ptr), v(cost2_ptr),
                                               v(evals_ptr), v(status_ptr), v(workspace_ptr)), "identify_device")

    # --- the wind identified jointly with the 21 --------------------------------
    def ident_sens_joint(self, x13, u3, wind, h: float, substeps: int = 4, params=None):
        """One sample interval per item under the wind (count, 3)
        (kite_nmpc_ident_sens_joint): x+ (count, 13) and S = d x+ / d (p, w)
        (count, 13, 24, unscaled): columns 0..20 ``IDENT_FIELDS``, 21..23 the wind."""
        x = _f64(x13).reshape(-1, 13); u = _f64(u3).reshape(-1, 3)
        c = x.shape[0]
        p = self._ident_rows(params, c)
        w = self._ident_wind(wind, c, None)
        xo = np.zeros((c, 13)); S = np.zeros((c, 13, IDENT_NPW))
        _check(lib().kite_nmpc_ident_sens_joint(self._h, c, float(h), int(substeps), ctypes.c_void_p(p.ctypes.data),
                                                p.shape[0], _p(x), _p(u), _p(w), _p(xo), _p(S)), "ident_sens_joint")
        return xo, S

    def _joint_logs(self, X, U, wind0):
        X = _f64(X); U = _f64(U)
        B, T = U.shape[0], U.shape[1]
        if X.shape != (B, T + 1, 13) or U.shape != (B, T, 3):
            raise ValueError("logs: X (B, T+1, 13), U (B, T, 3)")
        return X, U, B, T, (self._ident_wind(wind0, B, T) if wind0 is not None else None)

    def ident_normal_joint(self, X, U, p21, w3, params=None, config: Optional[IdentConfig] = None,
                           wind_config: Optional[IdentWindConfig] = None, wind0=None):
        """One evaluation of the joint normal equations at the parameter values
        p21 (B, 21) and the wind offset w3 (B, 3) (kite_nmpc_ident_normal_joint):
        (A (B, 24, 24), g (B, 24), cost (B,), status (B,)) in the scaled variables.
        wind0: the known wind log W0 (B, T, 3) or (B, 3), None: zeros; the model
        of sample k sees W0[k] + w."""
        cfg = config if config is not None else ident_default_config()
        wc = wind_config if wind_config is not None else ident_wind_default_config()
        X, U, B, T, W0 = self._joint_logs(X, U, wind0)
        p = self._ident_rows(params, B)
        q = _f64(p21).reshape(B, IDENT_NP)
        w = self._ident_wind(w3, B, None)
        A = np.zeros((B, IDENT_NPW, IDENT_NPW)); g = np.zeros((B, IDENT_NPW)); cost = np.zeros(B)
        st = np.zeros(B, dtype=np.int32)
        _check(lib().kite_nmpc_ident_normal_joint(self._h, ctypes.byref(cfg), ctypes.byref(wc), B, T,
                                                  ctypes.c_void_p(p.ctypes.data), p.shape[0], _p(q), _p(w), _p(X),
                                                  _p(U), _p(W0) if W0 is not None else None, _p(A), _p(g), _p(cost),
                                                  st.ctypes.data_as(_IP)), "ident_normal_joint")
        return A, g, cost, st

    def identify_joint(self, X, U, params=None, config: Optional[IdentConfig] = None,
                       wind_config: Optional[IdentWindConfig] = None, wind0=None) -> IdentResult:
        """Fit the 21 coefficients and a constant world-frame wind offset w of
        every kite to its log (kite_nmpc_identify_joint): for a fleet whose wind
        nobody knows.  wind0: a known wind log W0 (B, T, 3) or (B, 3) the offset
        is added to (a logged estimate whose bias is to be corrected), None:
        zeros.  Returns the ``IdentResult`` with ``wind`` (B, 3), the identified w."""
        cfg = config if config is not None else ident_default_config()
        wc = wind_config if wind_config is not None else ident_wind_default_config()
        X, U, B, T, W0 = self._joint_logs(X, U, wind0)
        p = self._ident_rows(params, B)
        out = np.zeros((B, len(_PARAM_FIELDS))); c2 = np.zeros((B, 2)); wo = np.zeros((B, 3))
        ev = np.zeros(B, dtype=np.int32); st = np.zeros(B, dtype=np.int32)
        _check(lib().kite_nmpc_identify_joint(self._h, ctypes.byref(cfg), ctypes.byref(wc), B, T,
                                              ctypes.c_void_p(p.ctypes.data), p.shape[0], _p(X), _p(U),
                                              _p(W0) if W0 is not None else None, ctypes.c_void_p(out.ctypes.data),
                                              _p(wo), _p(c2), ev.ctypes.data_as(_IP), st.ctypes.data_as(_IP)),
               "identify_joint")
        return IdentResult(out, c2[:, 0].copy(), c2[:, 1].copy(), ev, st, wo)

    def identify_joint_device(self, config: IdentConfig, wind_config: IdentWindConfig, count: int, T: int,
                              params_ptr: int, nparams: int, X_ptr: int, U_ptr: int, params_out_ptr: int,
                              wind_out_ptr: int, cost2_ptr: int = 0, evals_ptr: int = 0, status_ptr: int = 0,
                              workspace_ptr: int = 0, wind0: int = 0):
        """identify_joint on device pointers (kite_nmpc_identify_joint_device):
        2 * iters launches on the context stream, nothing allocated, copied or
        awaited; the workspace holds ``ident_joint_workspace_doubles`` doubles.
        wind0: device pointer of the known wind log (count, T, 3), 0: zeros."""
        v = lambda p: ctypes.c_void_p(p) if p else None
        _check(lib().kite_nmpc_identify_joint_device(self._h, ctypes.byref(config), ctypes.byref(wind_config),
                                                     int(count), int(T), v(params_ptr), int(nparams), v(X_ptr),
                                                     v(U_ptr), v(wind0), v(params_out_ptr), v(wind_out_ptr),
                                                     v(cost2_ptr), v(evals_ptr), v(status_ptr), v(workspace_ptr)),
               "identify_joint_device")

    def rk4_sens(self, x15, u4, tf: float, M: int):
        x = _f64(x15).reshape(-1, 15); u = _f64(u4).reshape(-1, 4)
        c = x.shape[0]
        xo = np.zeros((c, 15)); A = np.zeros((c, 15, 15)); Bm = np.zeros((c, 15, 4))
        _check(lib().kite_nmpc_rk4_sens(self._h, c, _p(x), _p(u), float(tf), int(M), _p(xo), _p(A), _p(Bm)),
               "rk4_sens")
        return xo, A, Bm


@dataclass
class _ReturnStatus:
    status: int

    @property
    def return_status(self) -> str:
        if self.status & ST_NAN:
            return "Invalid_Number_Detected"
        if self.status & ST_STEP_REJECTED:
            return "Restoration_Failed"
        if self.status & ST_QP_NOT_CONV:
            return "Maximum_Iterations_Exceeded"
        return "Solve_Succeeded"


def path_eval(config: NmpcConfig, theta):
    """P(theta) and dP/dtheta of the configured path (kite_nmpc_path_eval:
    getPathFunction, nmpf_node.cpp:30-40); host arithmetic, no GPU."""
    th = _f64(theta).reshape(-1)
    P = np.zeros((th.size, 3)); dP = np.zeros((th.size, 3))
    _check(lib().kite_nmpc_path_eval(ctypes.byref(config), th.size, _p(th), _p(P), _p(dP)), "path_eval")
    return P, dP


def score_combine(summaries) -> np.ndarray:
    """One raw summary (16,) from the raw summaries of several shards or ranks:
    slot by slot +, except max over SCORE_MAX_D and min over SCORE_MIN_SPEED,
    both over the summaries that scored a period (n > 0).  Host arithmetic."""
    S = [np.asarray(s, dtype=np.float64).reshape(SCORE_NSUM) for s in summaries]
    if not S:
        raise ValueError("score_combine: no summary")
    out = np.zeros(SCORE_NSUM)
    for s in S:                                     # in list order: reproducible
        out += s
    scored = [s for s in S if s[SCORE_N] > 0]
    out[SCORE_MAX_D] = max((s[SCORE_MAX_D] for s in scored), default=0.0)
    out[SCORE_MIN_SPEED] = min((s[SCORE_MIN_SPEED] for s in scored), default=0.0)
    return out


def score_derive(raw, dt: Optional[float] = None) -> dict:
    """The readable figures of a raw summary (16,): the raw slots by name
    (SCORE_SLOTS, slot 15 as "kites") and rms_d [m], mean_track, mean_u,
    mean_speed per scored period, mean_rate per period that has a predecessor,
    lost_fraction of all periods, kites_lost_fraction, laps (progress / 2 pi
    summed over the kites) and laps_per_kite; with dt [s] also lap_rate, the
    mean laps per second of flight between scored periods.  A ratio without
    a denominator is NaN."""
    raw = np.asarray(raw, dtype=np.float64).reshape(SCORE_NSUM)
    out = {name: float(raw[i]) for i, name in enumerate(SCORE_SLOTS[:15])}
    out["kites"] = float(raw[SCORE_KITES])

    def ratio(a, b):
        return float(a / b) if b > 0 else float("nan")
    n, nl, nr = raw[SCORE_N], raw[SCORE_N_LOST], raw[SCORE_N_RATE]
    out["rms_d"] = float(np.sqrt(ratio(raw[SCORE_SUM_D2], n)))
    out["mean_track"] = ratio(raw[SCORE_SUM_TRACK], n)
    out["mean_u"] = ratio(raw[SCORE_SUM_U], n)
    out["mean_speed"] = ratio(raw[SCORE_SUM_SPEED], n)
    out["mean_rate"] = ratio(raw[SCORE_SUM_RATE], nr)
    out["lost_fraction"] = ratio(nl, n + nl)
    out["kites_lost_fraction"] = ratio(raw[SCORE_EVER_LOST], raw[SCORE_KITES])
    out["laps"] = float(raw[SCORE_PROGRESS] / (2.0 * np.pi))
    out["laps_per_kite"] = ratio(raw[SCORE_PROGRESS] / (2.0 * np.pi), raw[SCORE_KITES])
    if dt is not None:
        out["lap_rate"] = ratio(raw[SCORE_PROGRESS] / (2.0 * np.pi), nr * dt)
    return out


def colloc_default_config(**overrides) -> CollocConfig:
    """The NMPF's collocation setup (kiteNMPF.cpp:80-143 + node scaling/path)."""
    c = CollocConfig()
    lib().kite_colloc_default_config(ctypes.byref(c))
    for k, v in overrides.items():
        cur = getattr(c, k)
        if hasattr(cur, "__len__"):
            for i, vi in enumerate(v):
                cur[i] = vi
        else:
            setattr(c, k, v)
    return c


def ekf_default_covariances():
    """(W, V, P0) of KiteEKF (kiteEKF.cpp:6-13, P0 = 10 W at :26)."""
    W = np.zeros((13, 13)); V = np.zeros((7, 7)); P0 = np.zeros((13, 13))
    lib().kite_ekf_default_covariances(_p(W), _p(V), _p(P0))
    return W, V, P0


def pose_frame_default() -> PoseFrame:
    """The reference node's motion-capture -> world frame (kite_pose_frame_default):
    offset (-0.09, 0, -0.02), rotation (0, -1, 0, 0), shift (0, 0, 2.77)."""
    f = PoseFrame()
    lib().kite_pose_frame_default(ctypes.byref(f))
    return f


def wind_ekf_default_covariances():
    """(W, V, P0) of the wind-estimating EKF, 16 x 16 / 7 x 7 / 16 x 16: the
    ``ekf_default_covariances`` blocks and the wind block of
    kite_windekf_default_covariances."""
    W = np.zeros((16, 16)); V = np.zeros((7, 7)); P0 = np.zeros((16, 16))
    lib().kite_windekf_default_covariances(_p(W), _p(V), _p(P0))
    return W, V, P0


class KiteEKF:
    """Mirror of the reference ``KiteEKF`` (kiteEKF.h:10-55) for a batch of
    kites on one GPU context: same setters/getters, ``propagate(dt)`` and
    ``_estimate(measurement, dt)``; ``estimate(measurement, tstamp)`` takes
    dt = tstamp - getTimeStamp() and, as in the reference (kiteEKF.cpp:100-105),
    leaves the time stamp to ``setTime``.

    model="kite" (the default) mirrors ``KiteEKF(KiteProperties,
    AlgorithmProperties)``: the filter with the kite's aerodynamic model.
    model="kinematic" mirrors ``KiteEKF(Function, Function)`` as the reference's
    estimator node builds it (ekf_node.cpp:235-241): the model-free filter of
    ``BatchNMPC.kin_ekf_step`` with ``substeps`` propagations per call and an
    optional pose ``frame``; ``setControl`` is accepted and ignored,
    ``initialize`` is the node's two-pose initialisation and ``status`` holds
    the KITE_EKF_* words of the last call."""

    def __init__(self, batch: int = 1, params: Optional[KiteParams] = None, device: int = 0, model: str = "kite",
                 substeps: int = 1, frame=None):
        if model not in ("kite", "kinematic"):
            raise ValueError('model is "kite" or "kinematic"')
        self._ctx = BatchNMPC(params if params is not None else load_properties(), default_config(device=device), batch)
        self.batch = batch
        self.model, self.substeps, self.frame = model, int(substeps), frame
        self.status = np.zeros(batch, dtype=np.int32)
        self.W, self.V, P0 = ekf_default_covariances()
        self.P = np.repeat(P0[None], batch, axis=0)
        self.x = np.zeros((batch, 13))
        self.u = np.zeros((batch, 3))
        self.tstamp = 0.0

    def close(self):
        self._ctx.close()

    def setProcessCovariance(self, W): self.W = _f64(W).reshape(13, 13).copy()
    def setMeasurementCovariance(self, V): self.V = _f64(V).reshape(7, 7).copy()
    def setEstimationCovariance(self, P): self.P = np.broadcast_to(_f64(P).reshape(-1, 13, 13), (self.batch, 13, 13)).copy()
    def setEstimation(self, x): self.x = np.broadcast_to(_f64(x).reshape(-1, 13), (self.batch, 13)).copy()
    def setControl(self, u): self.u = np.broadcast_to(_f64(u).reshape(-1, 3), (self.batch, 3)).copy()
    def setTime(self, t): self.tstamp = float(t)
    def getEstimation(self): return self.x.copy()
    def getEstimationCovariance(self): return self.P.copy()
    def getTimeStamp(self): return self.tstamp

    def propagate(self, dt: float):
        if self.model == "kinematic":
            self.x, self.P, self.status = self._ctx.kin_ekf_step(self.x, self.P, dt, self.substeps, None, self.W,
                                                                 self.V)
            return
        self.x, self.P = self._ctx.ekf_step(self.x, self.u, self.P, dt, None, self.W, self.V)

    def _estimate(self, measurement, dt: float):
        z = np.broadcast_to(_f64(measurement).reshape(-1, 7), (self.batch, 7))
        if self.model == "kinematic":
            self.x, self.P, self.status = self._ctx.kin_ekf_step(self.x, self.P, dt, self.substeps, z, self.W,
                                                                 self.V, self.frame)
            return
        self.x, self.P = self._ctx.ekf_step(self.x, self.u, self.P, dt, z, self.W, self.V)

    def initialize(self, pose_prev, pose_new, dt: float):
        """KiteEKF_Node::initialize (ekf_node.cpp:68-132), model="kinematic":
        the estimate from two consecutive poses dt apart, both through the
        frame; a kite that cannot be initialised keeps its estimate and has
        ``EKF_INIT_BAD`` in ``status``.  The time stamp is left to ``setTime``."""
        if self.model != "kinematic":
            raise ValueError('initialize belongs to KiteEKF(model="kinematic")')
        mp = np.broadcast_to(_f64(pose_prev).reshape(-1, 7), (self.batch, 7))
        mn = np.broadcast_to(_f64(pose_new).reshape(-1, 7), (self.batch, 7))
        self.x, self.status = self._ctx.kin_ekf_init(mp, mn, dt, self.frame, self.x)

    def estimate(self, measurement, tstamp: float):
        self._estimate(measurement, tstamp - self.tstamp)


class KiteNMPF:
    """Mirror of the reference ``KiteNMPF`` (kiteNMPF.h:10-118) for one kite.

    Setters / getters keep the reference names and semantics: matrices are
    returned in the reference's column order, i.e. time runs backwards and the
    LAST column of getOptimalControl() is u(t0) (nmpf_node.cpp:124).  The
    scaling matrices are diagonal; setReferenceVelocity is physical and, as
    in the reference, must be called after setStateScaling (it is stored in
    physical units here so the order no longer matters).
    """

    def __init__(self, params: Optional[KiteParams] = None, N: int = 20, dt: float = 0.05, **cfg):
        self._cfg = default_config(N=N, dt=dt, **cfg)
        self._params = params if params is not None else load_properties()
        self._impl: Optional[BatchNMPC] = None
        self._traj = None
        self._ctrl = None
        self._diag = None
        self._status = 0
        self._warm = False

    # setters kiteNMPF.h:20-34
    def setLBX(self, v): self._set("lbx", v)
    def setUBX(self, v): self._set("ubx", v)
    def setLBU(self, v): self._set("lbu", v)
    def setUBU(self, v): self._set("ubu", v)
    def setLBG(self, v): pass          # collocation equality bounds: no counterpart in the RTI
    def setUBG(self, v): pass

    def setStateScaling(self, S):
        self._set("Sx", np.diag(np.asarray(S, dtype=float)) if np.ndim(S) == 2 else S)

    def setControlScaling(self, S):
        self._set("Su", np.diag(np.asarray(S, dtype=float)) if np.ndim(S) == 2 else S)

    def setReferenceVelocity(self, v):
        self._cfg.vref = float(np.asarray(v).reshape(-1)[0])
        if self._impl is not None:
            self._impl.set_reference_velocity(self._cfg.vref)

    def setPath(self, radius: float, altitude: float = 0.0, q=(1.0, 0.0, 0.0, 0.0)):
        """The reference declares setPath(SX) but never defines it (kiteNMPF.h:36);
        the rotated circle of nmpf_node.cpp:30-40."""
        self._cfg.path_radius = radius
        self._cfg.path_altitude = altitude
        for i in range(4):
            self._cfg.path_q[i] = q[i]
        self._cfg.path_harmonics = 0
        self._impl = None

    def setPathFourier(self, coef, q=(1.0, 0.0, 0.0, 0.0)):
        """Any closed path (the path Function of KiteNMPF's ctor, kiteNMPF.h:14)
        as a rotated Fourier curve, see NmpcConfig.set_fourier_path."""
        self._cfg.set_fourier_path(coef, q)
        self._impl = None

    def _set(self, name, v):
        arr = getattr(self._cfg, name)
        for i, vi in enumerate(np.asarray(v, dtype=float).reshape(-1)):
            arr[i] = vi
        if self._impl is not None and name in ("lbx", "ubx", "lbu", "ubu"):
            self._impl.set_bounds(np.array(self._cfg.lbx), np.array(self._cfg.ubx),
                                  np.array(self._cfg.lbu), np.array(self._cfg.ubu))
        elif self._impl is not None:
            self._impl = None

    def createNLP(self):
        self._impl = BatchNMPC(self._params, self._cfg, 1)
        self._warm = False

    def enableWarmStart(self):
        self._warm = True

    def disableWarmStart(self):
        self._warm = False
        if self._impl is not None:
            self._impl.reset()

    def computeControl(self, X0):
        """KiteNMPF::computeControl (kiteNMPF.cpp:199-316) as one RTI step."""
        if self._impl is None:
            self.createNLP()
        if not self._warm:
            self._impl.reset()
        r = self._impl.step(np.asarray(X0, dtype=float).reshape(1, 15))
        self._traj, self._ctrl, self._diag, self._status = r["traj"][0], r["ctrl"][0], r["diag"][0], int(r["status"][0])
        self.enableWarmStart()

    def getOptimalControl(self):
        """4 x (N+1), reference shape and column order: column N - k = u_k (last
        column = u(t0)); column 0 (t = tf, where no interval starts) repeats
        u_{N-1}, the control held up to tf."""
        if self._ctrl is None:
            return None
        return np.vstack([self._ctrl, self._ctrl[-1:]])[::-1].T.copy()

    def getOptimalTrajetory(self):   # [sic] kiteNMPF.h:44
        """15 x (N+1), reference column order (last column = x(t0))."""
        return None if self._traj is None else self._traj[::-1].T.copy()

    def getPathFunction(self):
        """theta -> P(theta) (3,) of the configured path (kiteNMPF.h:46)."""
        cfg = self._cfg
        return lambda theta: path_eval(cfg, [theta])[0][0]

    def getStats(self):
        return {"return_status": _ReturnStatus(self._status).return_status, "status_bits": self._status}

    def getPathError(self):
        return 0.0 if self._diag is None else float(self._diag[0])

    def getVelocityError(self):
        return 0.0 if self._diag is None else float(self._diag[1])

    def getVirtState(self):
        return 0.0 if self._diag is None else float(self._diag[3])

    def initialized(self):
        return False   # never set true in the reference (kiteNMPF.cpp:46)

    def findClosestPointOnPath(self, position, init_guess=0.0):
        if self._impl is None:
            self.createNLP()
        return float(self._impl.closest_point(np.asarray(position, dtype=float).reshape(1, 3),
                                              np.array([float(init_guess)]))[0])

    def diagnostic(self):
        """mpc_diagnostic record (nmpf_node.cpp:191-204)."""
        return None if self._diag is None else dict(zip(DIAG_FIELDS, map(float, self._diag)))
