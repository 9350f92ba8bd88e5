"""openkite_amd -- MI355X-native batched NMPC (RTI) for the openKITE kite.

The product is libkite_nmpc.so (HIP kernels for gfx950 behind the C ABI in
include/kite_nmpc/kite_nmpc.h); this package is its Python host side.
"""
from .nmpc import (BatchNMPC, CollocConfig, KiteEKF, KiteNMPF, KiteNmpcError, KiteParams, NmpcConfig, MpcDiagnostic,  # noqa: F401
                   colloc_default_config, default_config, ekf_default_covariances, load_properties, lib, LIB_PATH, DIAG_FIELDS,
                   path_eval, perturb_params, resolve_qp_kernel, PERTURB_FIELDS, PLANT_NAN,
                   PLANT_CMD_DROPPED, PLANT_BAD_TAU, DELAY_DEPTH, DELAY_NLINE, DELAY_RULE, DELAY_RULE_SEQUENTIAL,
                   DELAY_RULE_TRANSPORT, ST_BAD_INFLIGHT, INFLIGHT_N,
                   wind_ekf_default_covariances, EKF_NAN, EKF_S_NOT_PD, WIND_MAX_DEFAULT,
                   EST_MODEL_CREATION, EST_MODEL_CONTROLLER, QP_SPLIT_AUTO, QP_SPLIT_NEVER, EKF_INIT_BAD, PoseFrame, pose_frame_default,
                   IdentConfig, IdentResult, ident_default_config, ident_param_index, ident_workspace_doubles,
                   save_properties, IDENT_FIELDS, IDENT_NP, IDENT_CHUNK, IDENT_NAN, IDENT_CONVERGED, IDENT_AT_BOUND,
                   IdentWindConfig, ident_wind_default_config, ident_joint_workspace_doubles, IDENT_WIND_AT_BOUND,
                   IDENT_NPW, score_combine, score_derive, SCORE_SLOTS, SCORE_NACC, SCORE_NSUM, SCORE_NMEM,
                   SCORE_N, SCORE_N_LOST, SCORE_EVER_LOST, SCORE_SUM_D2, SCORE_MAX_D, SCORE_SUM_TRACK, SCORE_SUM_U,
                   SCORE_SUM_RATE, SCORE_SUM_SPEED, SCORE_MIN_SPEED, SCORE_PROGRESS, SCORE_N_MIN_SPEED,
                   SCORE_N_QP_NOT_CONV, SCORE_N_STATE_BOUND, SCORE_N_RATE, SCORE_SPARE, SCORE_KITES,
                   SCORE_MEM_THETA, SCORE_MEM_U, SCORE_MEM_VALID)

__version__ = "0.1.0"
