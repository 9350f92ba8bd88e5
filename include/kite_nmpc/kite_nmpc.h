/*
 * kite_nmpc.h -- C ABI of the MI355X-native batched kite NMPC (RTI) library.
 *
 * This is the drop-in boundary for openKITE's NMPC hot path.  Each entry
 * point names the reference interface it replaces (paths relative to the
 * openKITE repository).  The reference exchanges casadi::DM objects; here
 * every matrix is a plain row-major double array, batched over independent
 * NMPC instances ("batch" B).  No torch / HIP types appear in the signatures
 * except an opaque stream handle (void*).
 *
 * Conventions
 *   - Return 0 (KITE_OK) on success, a negative KITE_E* code otherwise.
 *     Per-instance solver trouble never fails a call: it is reported in the
 *     int32 status word of that instance (KITE_ST_* bits).
 *   - "host" entry points take host pointers and copy in/out (synchronous).
 *     "_device" entry points take device pointers and are asynchronous on the
 *     context stream (kite_nmpc_set_stream).
 *   - One context per host thread; a context is not re-entrant.  Contexts on
 *     different devices are independent (that is how the batch shards over
 *     GPUs: one process and one context per GPU).
 *   - There is no CPU fallback: kite_nmpc_create fails with KITE_ENODEV when
 *     no gfx950 device is usable.
 *
 * Time ordering: arrays run FORWARD in time (node 0 = t0).  The reference's
 * Chebyshev nodes run backwards (node N = t0, chebyshev.hpp:119-127,
 * kiteNMPF.cpp:232-235); the C++ facade KiteNMPF.hpp restores that column
 * order for getOptimalControl()/getOptimalTrajetory().
 */
#ifndef KITE_NMPC_H
#define KITE_NMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KITE_NMPC_API_VERSION 7   /* 2: kite_nmpc_config gained qp_soft_weight, qp_lm;
                                      qp_kernel 3 (multiple-shooting QP, Riccati IPM);
                                   3: kite_nmpc_config gained path_harmonics, path_fourier
                                      (arbitrary closed paths); delay_steps default 16;
                                   4: kite_nmpc_state_bound_stats (no config change);
                                   5: kite_nmpc_set_wind (no config change);
                                   6: kernel_times / timing_read report a sixth
                                      entry, the main QP kernel alone;
                                   7: kite_nmpc_timing_start_sampled (events on
                                      every stride-th step; no config change);
                                      additive, no version change: the plant
                                      simulator (kite_nmpc_plant_set_params,
                                      _plant_set_wind, _plant_step, _plant_step_device,
                                      KITE_PLANT_NAN) and the wind-estimating EKF
                                      (kite_nmpc_windekf_step[_device], _jacobian_wind,
                                      _set_wind_device, KITE_EKF_*) and the parameter
                                      identification (kite_nmpc_identify[_device],
                                      _ident_normal, _ident_sens, KITE_IDENT_*) and
                                      the per-kite controller models
                                      (kite_nmpc_set_params[_device], _get_params,
                                      KITE_PARAMS_REJECTED) and the estimators' model
                                      (kite_nmpc_set/get_estimator_model,
                                      KITE_EST_MODEL_*) and the identification under
                                      a logged wind (kite_nmpc_identify_wind[_device],
                                      _ident_normal_wind, _ident_sens_wind) and the
                                      kinematic EKF (kite_nmpc_kinekf_step[_device],
                                      _kinekf_init[_device], _jacobian_kin,
                                      kite_pose_frame, KITE_EKF_INIT_BAD) and the
                                      wind identified jointly with the 21
                                      (kite_nmpc_identify_joint[_device],
                                      _ident_normal_joint, _ident_sens_joint,
                                      kite_ident_wind_config,
                                      KITE_IDENT_WIND_AT_BOUND) and the actuation
                                      delay (kite_nmpc_plant_step_delayed[_device],
                                      KITE_DELAY_*, KITE_PLANT_CMD_DROPPED,
                                      KITE_PLANT_BAD_TAU) and the line's transport
                                      rule and the in-flight schedule
                                      (KITE_DELAY_RULE*, kite_nmpc_set_inflight[_device],
                                      _get_inflight, KITE_INFLIGHT_N,
                                      KITE_ST_BAD_INFLIGHT)                       */
#define KITE_PATH_MAX_HARMONICS 8 /* Fourier path: harmonics per axis              */

/* ---- error codes ------------------------------------------------------ */
#define KITE_OK        0
#define KITE_EINVAL   (-1)   /* bad argument                                  */
#define KITE_EHIP     (-2)   /* HIP runtime error                             */
#define KITE_ENOMEM   (-3)   /* device or host allocation failed              */
#define KITE_ENODEV   (-4)   /* no usable gfx950 device                       */
#define KITE_EIO      (-5)   /* parameter file cannot be read                 */
#define KITE_EPARSE   (-6)   /* parameter file lacks a key / bad number       */
#define KITE_ESTATE   (-7)   /* call not valid in this context state          */

/* ---- per-instance status bits (status_out) ---------------------------- */
#define KITE_ST_NAN            1   /* non-finite value in the new iterate     */
#define KITE_ST_QP_NOT_CONV    2   /* QP residual > 1e-8 after the cap K       */
#define KITE_ST_MIN_SPEED      4   /* vx clamped to min_speed (nmpf_node.cpp:241-243) */
#define KITE_ST_STATE_BOUND    8   /* new trajectory still outside lbx/ubx after the
                                      lazy state-bound rows (vx: a QP row at every
                                      node; states 1..12: at most 4 rows per step,
                                      2 re-solves -- DESIGN.md 4.4)                */
#define KITE_ST_THETA_WRAP    16   /* theta wrapped by 2*pi (kiteNMPF.cpp:212-221) */
#define KITE_ST_STEP_REJECTED 32   /* QP residual >= 1e-6 or NaN: no step applied, the
                                      shifted plan is kept (the reference applies the
                                      failed iterate, kiteNMPF.cpp:303-313)          */
#define KITE_ST_RESTART       64   /* the warm start held non-finite values: this kite
                                      was restarted cold, theta from the closest point
                                      and thetadot = 0 (nmpf_node.cpp:225-236)        */
#define KITE_ST_BAD_INFLIGHT 128   /* the kite's in-flight schedule row is invalid (n = -1,
                                      kite_nmpc_set_inflight): the delay compensation
                                      predicted under the previous u(t0) instead        */

/* ---- model parameters: kite_utils::LoadProperties (kite.cpp:7-76) ------
 * Field order == KiteProperties (kite.h:9-93) flattened.  52 doubles.     */
typedef struct kite_params {
    /* geometry */
    double b, c, AR, S, lam, St, lt, Sf, lf, Xac;
    /* inertia */
    double mass, Ixx, Iyy, Izz, Ixz;
    /* aerodynamics */
    double CL0, CL0_tail, CLa_total, CLa_wing, CLa_tail, e_oswald;
    double CD0_total, CD0_wing, CD0_tail, CYb, CYb_vtail, Cm0, Cma;
    double Cn0, Cnb, Cl0, Clb, CLq, Cmq, CYr, Cnr, Clr, CYp, Clp, Cnp;
    double CLde, CYdr, Cmde, Cndr, Cldr, CDde;
    /* tether */
    double Lt, Ks, Kd, rx, ry, rz;
} kite_params;

/* ---- controller configuration ------------------------------------------
 * Replaces the KiteNMPF ctor + setters + createNLP (kiteNMPF.h:14-37,
 * kiteNMPF.cpp:18-197) and the values the ROS node feeds them
 * (nmpf_node.cpp:30-69).  Units are physical; Sx/Su are the diagonals of the
 * reference scaling matrices (setStateScaling / setControlScaling).      */
typedef struct kite_nmpc_config {
    int32_t N;            /* shooting intervals (20; 40 for long horizons)     */
    int32_t M;            /* RK4 substeps per interval (2)                     */
    int32_t qp_iters;     /* interior-point iteration cap K (16)               */
    int32_t shift;        /* 1: shift the warm start by one interval per step  */
    int32_t device;       /* HIP device ordinal                                 */
    int32_t timing;       /* 1: record per-kernel hipEvents (kite_nmpc_kernel_times) */
    int32_t qp_kernel;    /* 0: auto (2 at N == 20, else 3), 1: condensed QP, wave-scalar LDS IPM,
                             2: condensed QP, MFMA-tiled IPM (register tiles at N == 20, LDS
                             tiles with 4 waves per kite at N == 40; KITE_EINVAL otherwise),
                             3: multiple-shooting QP (every node state a variable, as the
                             reference NLP kiteNMPF.cpp:145-160), Riccati IPM on MFMA tiles,
                             soft state bounds (qp_soft_weight) and a Levenberg-Marquardt
                             term (qp_lm).  1 and 2 enforce the state bounds of states 1..12
                             as lazy rows. */
    int32_t delay_steps;  /* RK4 substeps of the delay-compensation prediction (16) */
    double dt;            /* interval length [s] (0.05 -> tf = 1 s at N = 20)  */
    double Q[3];          /* path weights  (kiteNMPF.cpp:32)                   */
    double R[4];          /* control weights (kiteNMPF.cpp:33)                 */
    double W;             /* path-speed weight (kiteNMPF.cpp:34)               */
    double Sx[15], Su[4]; /* scaling diagonals (nmpf_node.cpp:50-51)           */
    double lbx[15], ubx[15];  /* state bounds (nmpf_node.cpp:59-63); +-INFINITY = none;
                                 13, 14 (theta, thetadot) are not bounded    */
    double lbu[4], ubu[4];    /* control bounds (nmpf_node.cpp:45-47)          */
    double vref;          /* physical path speed (setReferenceVelocity, nmpf_node.cpp:68) */
    double path_radius;   /* P(theta) = rot(q)[R cos, R sin, alt] (nmpf_node.cpp:30-40)
                             when path_harmonics == 0 (see path_fourier)             */
    double path_altitude;
    double path_q[4];     /* (w,x,y,z); P = vec(q^-1 (x) p (x) q)               */
    double theta_flex;    /* +- relaxation of theta, thetadot at t0 (kiteNMPF.cpp:226) */
    double min_speed;     /* caller-side vx clamp (nmpf_node.cpp:241-243); <= -INF disables */
    double delay;         /* transport-delay compensation of the ROS node, fused into
                             the step (nmpf_node.cpp:206-221): on warm steps the kite
                             part of x0 is predicted over `delay` s under the previous
                             u(t0) (RK4, delay_steps substeps; the node used CVODES,
                             abstol 1e-4: 16 substeps stay within 2e-5)
                             and theta, thetadot are taken from the previous trajectory
                             at node round(delay/dt).  0 = off: KiteNMPF semantics, the
                             caller passes the predicted state (default).  The node
                             uses 0.1 (nmpf_node.cpp:74).  With an in-flight schedule
                             (kite_nmpc_set_inflight) the prediction runs under the
                             commands still in the line, piecewise constant.           */
    int32_t sens_fp32;    /* 1: RK4 + forward sensitivities in fp32 (mixed precision,
                             BASELINE config 4); condensing, QP, expansion stay fp64 */
    int32_t reserved;
    double qp_soft_weight; /* qp_kernel 3: exact-L1 weight of the state bounds in the reference's
                              scaled units (1e3); the QP stays feasible when the linearised
                              dynamics cannot meet the box over the horizon.  Must exceed
                              40 = 2 z0 (the IPM's start multiplier, so every soft row starts
                              dual feasible): smaller values give KITE_EINVAL                 */
    double qp_lm;          /* qp_kernel 3: Levenberg-Marquardt term lm/2 ||step||^2 on every QP
                              variable, scaled units (10); leaves the RTI fixed point unchanged.
                              qp_lm = 0 with qp_soft_weight = 1e6 at N = 20: the condensed
                              QP's own step with the state box exact on every node
                              (DESIGN.md 4.4); at N = 40 the undamped step diverges        */
    /* Arbitrary closed path (KiteNMPF(kite, path), kiteNMPF.h:14, takes any
     * casadi::Function theta -> R^3): with path_harmonics = K in 1..8 the
     * unrotated curve is the truncated Fourier series
     *   p_a(theta) = F[a][0] + sum_{k=1..K} F[a][2k-1] cos(k theta) + F[a][2k] sin(k theta)
     * per axis a = x, y, z, and P(theta) = vec(q^-1 (x) [0, p] (x) q) with path_q
     * as for the circle (path_radius / path_altitude are then unused).  The
     * circle is K = 1, F[0][1] = F[1][2] = R, F[2][0] = alt.  0 (default): the
     * circle.  Every path evaluation of the step (closest point, residuals,
     * diagnostics, kite_nmpc_path_eval) uses it.                               */
    int32_t path_harmonics;
    int32_t reserved2;
    double path_fourier[3][2 * KITE_PATH_MAX_HARMONICS + 1];
} kite_nmpc_config;

/* ---- diagnostics: msg/mpc_diagnostic.msg (filled at nmpf_node.cpp:191-204) */
typedef struct kite_mpc_diagnostic {
    double pos_error;     /* ||Sr (P(theta0) - r0)||  (kiteNMPF.cpp:319-330)    */
    double vel_error;     /* |Sx14 (vref - thetadot0)| (kiteNMPF.cpp:333-344)   */
    double cost;          /* objective of the new iterate (reference sends 0)  */
    double virt_state;    /* theta at t0 (kiteNMPF.cpp:347-355)                 */
    double virt_ctrl;     /* Uv at t0 (unset in the reference)                  */
    double comp_time_ms;  /* host-measured step time of the whole batch         */
} kite_mpc_diagnostic;

typedef struct kite_nmpc_ctx kite_nmpc_ctx;

/* kite_utils::LoadProperties (kite.cpp:7-76).  Unlike the reference, a
 * missing tether.rx/ry/rz defaults to 0 (the shipped umx_radian.yaml lacks
 * them); any other missing key is KITE_EPARSE.              */
int kite_params_load_yaml(const char* path, kite_params* out);

/* Node defaults: nmpf_node.cpp:30-69 + kiteNMPF.cpp:32-34 + RTI settings.  */
void kite_nmpc_default_config(kite_nmpc_config* cfg);

/* KiteNMPF ctor + setters + createNLP (kiteNMPF.cpp:18-197).  Allocates all
 * device buffers for `batch` instances on cfg->device.                      */
int kite_nmpc_create(const kite_params* params, const kite_nmpc_config* cfg,
                     int32_t batch, kite_nmpc_ctx** out);
void kite_nmpc_destroy(kite_nmpc_ctx* ctx);
const char* kite_nmpc_strerror(int code);

/* setLBX/setUBX/setLBU/setUBU (kiteNMPF.h:20-27).  NULL keeps a vector.     */
int kite_nmpc_set_bounds(kite_nmpc_ctx* ctx, const double* lbx15, const double* ubx15,
                         const double* lbu4, const double* ubu4);
/* setReferenceVelocity (kiteNMPF.h:34); physical units.                     */
int kite_nmpc_set_reference_velocity(kite_nmpc_ctx* ctx, double vref);
/* disableWarmStart (kiteNMPF.h:40): the next step cold-starts.              */
int kite_nmpc_reset(kite_nmpc_ctx* ctx);
/* Wind-field sweeps (the batch dimension of BASELINE north_star): a constant
 * world-frame wind per instance, wind[3 b + i] in m/s (B x 3), or NULL for
 * none.  Build extension: the reference model has no wind (kite.cpp:196
 * "@todo: add wind"); with wind the RTI model's aerodynamics see the
 * air-relative velocity v - q^-1 W q (kite_model.hpp), used by every step's
 * prediction (cold start, delay compensation, sensitivities, defects).  The
 * item-wise model entry points (dynamics, jacobian, predict, rk4_sens) and
 * the EKF keep the reference model.  All-zero wind is the reference model
 * bit for bit.  Non-finite entries: KITE_EINVAL.                            */
int kite_nmpc_set_wind(kite_nmpc_ctx* ctx, const double* wind);
/* Run on this HIP stream (hipStream_t as void*).  NULL is the HIP null
 * (legacy default) stream -- the stream PyTorch's default stream maps to.
 * A new context runs on a private non-blocking stream; restore it with
 * kite_nmpc_use_own_stream.                                                  */
int kite_nmpc_set_stream(kite_nmpc_ctx* ctx, void* hip_stream);
int kite_nmpc_use_own_stream(kite_nmpc_ctx* ctx);
int kite_nmpc_synchronize(kite_nmpc_ctx* ctx);

/* findClosestPointOnPath (kiteNMPF.cpp:358-391), batched over `count`
 * positions (count x 3); guess may be NULL (= 0 as in the reference).       */
int kite_nmpc_closest_point(kite_nmpc_ctx* ctx, int32_t count, const double* pos,
                            const double* guess, double* theta_out);
/* getPathFunction (kiteNMPF.h:46; the path built at nmpf_node.cpp:30-40 and
 * evaluated per trajectory node for /opt_traj at nmpf_node.cpp:177-183):
 * P(theta) = vec(q^-1 (x) [0, p(theta)] (x) q) (the circle p = [R cos, R sin,
 * alt] or the Fourier curve of path_harmonics) and dP/dtheta for
 * `count` angles (count x 3 each; dP3 may be NULL).  Host arithmetic on the
 * configuration only (no context, no GPU): a visualisation helper of the
 * node, not part of the RTI step.                                           */
int kite_nmpc_path_eval(const kite_nmpc_config* cfg, int32_t count, const double* theta,
                        double* P3, double* dP3);

/* One RTI step for the whole batch: replaces KiteNMPF::computeControl
 * (kiteNMPF.cpp:199-316) -- NLP_Solver(ARG) becomes shift -> rk4_sens ->
 * condense -> QP -> expand.
 *   x0        B x 15 augmented state [v w r q theta thetadot] (physical)
 *   u0_out    B x 4  control to apply = last column of getOptimalControl()
 *   traj_out  B x (N+1) x 15 optimal trajectory (forward time), nullable
 *   ctrl_out  B x N x 4 optimal controls, nullable
 *   diag_out  B mpc_diagnostic records, nullable
 *   status_out B status words, nullable                                      */
int kite_nmpc_step(kite_nmpc_ctx* ctx, const double* x0, double* u0_out,
                   double* traj_out, double* ctrl_out, kite_mpc_diagnostic* diag_out,
                   int32_t* status_out);
/* Same, device pointers, asynchronous on the context stream.  diag_out is
 * B x 6 doubles in kite_mpc_diagnostic order (comp_time_ms left 0).          */
int kite_nmpc_step_device(kite_nmpc_ctx* ctx, const double* d_x0, double* d_u0,
                          double* d_traj, double* d_ctrl, double* d_diag, int32_t* d_status);

/* Warm-start access (getOptimalTrajetory / getOptimalControl state, and
 * NLP_X warm start injection).  Host pointers, B x (N+1) x 15 and B x N x 4. */
int kite_nmpc_get_solution(kite_nmpc_ctx* ctx, double* traj, double* ctrl);
int kite_nmpc_set_solution(kite_nmpc_ctx* ctx, const double* traj, const double* ctrl);

/* ---- model-level entry points (KiteDynamics, kite.cpp:320-338) ---------- */
/* getNumericDynamics: f(x,u), count x 15 states (augmented), count x 4 ctrl. */
int kite_nmpc_dynamics(kite_nmpc_ctx* ctx, int32_t count, const double* x15,
                       const double* u4, double* f15);
/* getNumericJacobian: df/dx (13 x 13) and df/du (13 x 3) of the kite ODE.    */
int kite_nmpc_jacobian(kite_nmpc_ctx* ctx, int32_t count, const double* x13,
                       const double* u3, double* Jx, double* Ju);
/* RK4 integrator (kitemath.cpp:36-51, integrator.cpp:86-98) with `steps`
 * substeps over tf: the delay-compensation predictor of nmpf_node.cpp:218.   */
int kite_nmpc_predict(kite_nmpc_ctx* ctx, int32_t count, const double* x15,
                      const double* u4, double tf, int32_t steps, double* x15_out);
/* The hot kernel alone (k_rk4_sens2 on `count` one-interval horizons, BASELINE
 * config 2): x+ and S = dx+/d[x,u] over one shooting interval (h = tf/M, M
 * substeps).  count x 15, count x 4 -> count x 15, count x 15 x 15,
 * count x 15 x 4.  Sensitivities in fp32 (x+ in fp64) when the context was
 * created with config.sens_fp32 = 1.                                        */
int kite_nmpc_rk4_sens(kite_nmpc_ctx* ctx, int32_t count, const double* x15,
                       const double* u4, double tf, int32_t M, double* xnext,
                       double* A, double* B);

/* ---- plant simulator (src/kite_model/simulator.cpp) ----------------------
 * The plant the controller is flown against: the kite ODE of every instance
 * integrated on the device under the held control, with a plant model, a wind
 * and a gust per kite that the controller is not told about (model-plant
 * mismatch).  The context owns the device copies of the plant constants and
 * the plant wind.  With neither set the plant is the controller's own model
 * without wind, i.e. what kite_nmpc_predict integrates.                     */
#define KITE_PLANT_NAN 1   /* plant status bit: state went non-finite, kite frozen */

/* Per-kite plant model.  count == batch: params[b] is kite b's plant;
 * count == 1: one plant model for all; params == NULL: the controller's own
 * parameters (the default).  Anything else, a non-finite field, mass <= 0 or a
 * singular inertia matrix: KITE_EINVAL, and the previous setting is kept.     */
int kite_nmpc_plant_set_params(kite_nmpc_ctx* ctx, const kite_params* params, int32_t count);

/* Per-kite plant wind, B x 8: [W0x W0y W0z  Ax Ay Az  f_hz  phase_rad], world
 * frame, m/s: W(t) = W0 + A sin(2 pi f t + phase).  NULL: none.  Independent
 * of kite_nmpc_set_wind (what the controller's model assumes).  Non-finite
 * entries: KITE_EINVAL, and the previous setting is kept.                    */
int kite_nmpc_plant_set_wind(kite_nmpc_ctx* ctx, const double* wind8);

/* Advance every kite's 13 plant states in place from time t0 over steps * h
 * under the held control u4 (B x 4; T, dE, dR; the 4th is ignored), RK4 with
 * `substeps` per step (simulator.cpp:43-51; the driver uses h = 0.02, 4).
 * Substep k of the call starts at t0 + k (h / substeps): a call that starts
 * where another ended continues it.  status (nullable): B words of
 * KITE_PLANT_* bits, written (not OR-ed) on every call.  A kite whose state
 * turns non-finite keeps its last finite state and is flagged; one that is
 * non-finite on entry is left untouched and flagged.  h <= 0 or non-finite,
 * steps < 1, substeps < 1, steps * substeps > 2^24, non-finite t0:
 * KITE_EINVAL.                                                              */
int kite_nmpc_plant_step(kite_nmpc_ctx* ctx, double* x13, const double* u4, double t0,
                         double h, int32_t steps, int32_t substeps, int32_t* status);
/* Same on device pointers, asynchronous on the context stream.              */
int kite_nmpc_plant_step_device(kite_nmpc_ctx* ctx, double* d_x13, const double* d_u4, double t0,
                                double h, int32_t steps, int32_t substeps, int32_t* d_status);

/* ---- actuation delay: a command line per kite ----------------------------
 * The plant behind the reference's transport delay (src/nodes/
 * transport_delay.cpp, a FIFO channel; simulator.cpp flies whatever command it
 * received last).  Every kite owns a LINE of KITE_DELAY_NLINE doubles, kept by
 * the caller: the control in force and a FIFO of at most KITE_DELAY_DEPTH
 * pending commands with their arrival times.  An all-zero line is a reset:
 * empty FIFO, zero control in force, no previous arrival.
 *
 * One call is one control period of `steps` plant steps of h, per kite:
 *   send    u4_cmd[b] (if given) is sent at t_send = t0 with latency tau[b]:
 *           t_arr = max(t_send, t_arr_prev) + tau[b], t_arr_prev the arrival of
 *           the kite's last accepted command (t_send if there is none): the
 *           channel never reorders.  tau[b] negative or non-finite: the
 *           command is dropped, KITE_PLANT_BAD_TAU.  A send to a full line
 *           drops the OLDEST pending command, KITE_PLANT_CMD_DROPPED.
 *           That is KITE_DELAY_RULE_SEQUENTIAL: every accepted command is
 *           charged its latency after the one before it, so a latency above
 *           the control period makes the line fall behind.  A line whose
 *           KITE_DELAY_RULE slot holds exactly 1.0 (KITE_DELAY_RULE_TRANSPORT)
 *           takes t_arr = max(t_send + tau[b], t_arr_prev) instead (t_arr_prev
 *           only once a command has been accepted): a pure transport delay,
 *           clamped so that the channel still never reorders.  Everything else
 *           of the send is the same under both rules; the rule is per line,
 *           the caller writes the slot and the calls carry it through.
 *   fly     before plant step j (j = 0 .. steps-1) every pending command with
 *           t_arr <= t_j leaves the FIFO in order and the last of them becomes
 *           the control in force; t_j = t0 + (double)(j * substeps) * (h /
 *           substeps), product rounded, then the sum.  The step then runs its
 *           RK4 substeps as kite_nmpc_plant_step does.  Commands take effect at
 *           plant ticks only; a step is never split.
 *   report  u4_applied[b] is the control in force during the call's last plant
 *           step; status[b] (written, not OR-ed) holds KITE_PLANT_* bits.  The
 *           line advances whether or not the kite's state is finite.
 *
 * Line slots (doubles):                                                      */
#define KITE_DELAY_DEPTH        4
#define KITE_DELAY_NLINE        32   /* doubles per kite; all zero = reset */
#define KITE_DELAY_COUNT        0    /* pending commands, 0 .. KITE_DELAY_DEPTH           */
#define KITE_DELAY_T_PREV       1    /* arrival time of the last accepted command         */
#define KITE_DELAY_HAS_PREV     2    /* 1 once a command has been accepted, else 0        */
#define KITE_DELAY_RULE         3    /* the arrival rule: exactly 1.0 is KITE_DELAY_RULE_TRANSPORT,
                                        any other value (NaN included) _SEQUENTIAL       */
#define KITE_DELAY_RULE_SEQUENTIAL 0 /* t_arr = max(t_send, t_arr_prev) + tau             */
#define KITE_DELAY_RULE_TRANSPORT  1 /* t_arr = max(t_send + tau, t_arr_prev)             */
#define KITE_DELAY_U_FORCE      4    /* 4..7: the control in force (T, dE, dR, 4th)       */
#define KITE_DELAY_T_ARR        8    /* 8..11: arrival times, slot 0 the oldest           */
#define KITE_DELAY_U            12   /* 12..27: the pending commands, 4 doubles per slot  */
                                     /* 28..31: reserved, zero; free slots are zero       */
#define KITE_PLANT_CMD_DROPPED  2    /* plant status bit: a full line dropped its oldest command */
#define KITE_PLANT_BAD_TAU      4    /* plant status bit: tau negative or non-finite, command dropped */

/* x13, tau (B), line (B x KITE_DELAY_NLINE, in place), u4_applied (B x 4,
 * nullable), status (B, nullable).  u4_cmd (B x 4) NULL: nothing is sent this
 * period (tau may then be NULL).  The plant parameters, wind and gust are those
 * of kite_nmpc_plant_set_params / _set_wind.  kite_nmpc_plant_step's argument
 * checks, and line == NULL, or tau == NULL with a command: KITE_EINVAL, and
 * nothing is changed.                                                        */
int kite_nmpc_plant_step_delayed(kite_nmpc_ctx* ctx, double* x13, const double* u4_cmd, const double* tau,
                                 double* line, double* u4_applied, double t0, double h, int32_t steps,
                                 int32_t substeps, int32_t* status);
/* Same on device pointers, asynchronous on the context stream.              */
int kite_nmpc_plant_step_delayed_device(kite_nmpc_ctx* ctx, double* d_x13, const double* d_u4_cmd,
                                        const double* d_tau, double* d_line, double* d_u4_applied, double t0,
                                        double h, int32_t steps, int32_t substeps, int32_t* d_status);

/* ---- the in-flight schedule: the line as the controller sees it -----------
 * The delay compensation (config.delay) predicts the measured state over the
 * delay under ONE control, the previous u(t0).  With a latency above one
 * control period the line holds several different commands.  The in-flight
 * schedule is a snapshot of every kite's line at time t0, kept by the context:
 * a row of KITE_INFLIGHT_N doubles per kite,
 *   [0]      n, the number of switches: the pending count as the send reads it
 *            (0 .. KITE_DELAY_DEPTH, NaN read as 0), or -1: the row is invalid
 *   [1..4]   s_i, seconds after t0 at which pending command i takes over:
 *            max(t_arr_i - t0, 0), then a running maximum over i (the FIFO pops
 *            in order)
 *   [5..7]   the control in force (T, dE, dR)
 *   [8..19]  the pending commands (T, dE, dR), oldest first
 *   rest     zero; unused entries are zero
 * A non-finite control in force, or a non-finite arrival time or (T, dE, dR) of
 * one of the n pending commands, makes the row invalid: n = -1, the rest zero.
 * The 4th control of a command is not part of the kite model and is ignored.
 *
 * With a schedule set, a warm step with config.delay = D > 0 predicts every
 * kite with a valid row over [0, D] under the piecewise-constant control: the
 * control in force until s_1, command i from s_i until s_{i+1}, the last to D.
 * Switches with s_i >= D are ignored and zero-length pieces are skipped (a
 * command superseded at the same instant never flies).  A piece of length L
 * takes n RK4 substeps of L / n, n the smallest integer in 1 .. delay_steps
 * with (double)n * (D / delay_steps) >= L (delay_steps if there is none): a
 * window without a switch is the prediction without a schedule, bit for bit.
 * A kite with an invalid row is predicted under the previous u(t0) and flagged
 * KITE_ST_BAD_INFLIGHT.  Cold steps have no compensation and ignore it.
 *
 * The schedule stays in force, as stored, until it is replaced or switched
 * off with NULL; kite_nmpc_reset keeps it.  The caller refreshes it every
 * period, right before the step.  config.delay == 0 with a schedule, or
 * _get_inflight without one: KITE_ESTATE, nothing changes.  Non-finite t0:
 * KITE_EINVAL.  The switch times are the arrival instants; the plant applies a
 * command at its next tick (see above), a gap of less than one plant step.  */
#define KITE_INFLIGHT_N 24  /* doubles per kite */
/* d_line: B x KITE_DELAY_NLINE in device memory (read in stream order, not
 * changed), asynchronous on the context stream.                             */
int kite_nmpc_set_inflight_device(kite_nmpc_ctx* ctx, const double* d_line, double t0);
/* Same, host pointer.                                                       */
int kite_nmpc_set_inflight(kite_nmpc_ctx* ctx, const double* line, double t0);
/* The schedule rows in force, B x KITE_INFLIGHT_N (host pointer; tests).    */
int kite_nmpc_get_inflight(kite_nmpc_ctx* ctx, double* sched);

/* ---- introspection (tests, profiling) ---------------------------------- */
/* ---- reference formulation: Chebyshev collocation (chebyshev.hpp) -------
 * Evaluates the reference's own NLP functions for `count` points
 * z = [X (nodes x 15) | U (nodes x 4)], nodes = poly_order*num_segments + 1,
 * in the reference's (optionally scaled) variables:
 *   G = (CompDiff (x) I15) X - t_scale * SODE(X_i, U_i)      (chebyshev.hpp:241-271)
 *   J = mayer_scale * M(X_0) + sum_seg t_scale sum_m w_m L(X, U) (:280-333)
 * with t_scale = (tf - t0) / (2 num_segments), SODE(x, u) = Sx f_aug(x/Sx, u/Su)
 * (kiteNMPF.cpp:100-104), L = Q.res^2 + W (vref - x14)^2 [+ R.u^2],
 * res = Sx_r P(x13 / Sx13) - x(6:9), M = Q.res^2 (kiteNMPF.cpp:117-143).
 * jac (nullable): per node the 15 x 19 block d SODE / d [x, u] at (X_i, U_i);
 * the constraint Jacobian is dG/dX = CompDiff (x) I - t_scale blockdiag(jac_x),
 * dG/dU = -t_scale blockdiag(jac_u).                                         */
typedef struct kite_colloc_config {
    int32_t poly_order;     /* 5 (kiteNMPF.cpp:83); 10 in full_generics_test     */
    int32_t num_segments;   /* 2 (kiteNMPF.cpp:82); 1 in full_generics_test      */
    int32_t use_R;          /* 1: L includes R u^2 (NMPF); 0: full_generics_test */
    int32_t reserved;
    double t0, tf;
    double Q[3], R[4], W;
    double vref;            /* in the formulation's variables (Sx14 * v when scaled) */
    double mayer_scale;     /* 1 (NMPF), 2 (full_generics_test)                   */
    double Sx[15], Su[4];   /* 1 = unscaled                                       */
    double path_radius, path_altitude, path_q[4];
    int32_t path_harmonics;  /* as kite_nmpc_config (API 3): 0 the circle, 1..8 Fourier path */
    int32_t reserved2;
    double path_fourier[3][2 * KITE_PATH_MAX_HARMONICS + 1];
} kite_colloc_config;
/* The NMPF's setup (kiteNMPF.cpp:80-143 with the node's scaling and path).  */
void kite_colloc_default_config(kite_colloc_config* cfg);
int kite_nmpc_colloc_eval(kite_nmpc_ctx* ctx, const kite_colloc_config* cfg, int32_t count, const double* z,
                          double* G, double* J, double* jac);

/* ---- extended Kalman filter: KiteEKF (src/kite_estimation/kiteEKF.cpp) ---
 * For each of `count` kites: propagate(dt) (kiteEKF.cpp:75-98: one RK4 step,
 * A = I + J dt, P = A P A' + W) and, when z7 != NULL, the update of
 * _estimate (kiteEKF.cpp:108-126) with H = [0_{7x6} I_7] (position r and
 * quaternion q measured).  x13 (count x 13) and P169 (count x 13 x 13,
 * row-major) are updated in place; u3 count x 3 (T, dE, dR); z7 count x 7;
 * W169 / V49 shared by all kites.                                           */
void kite_ekf_default_covariances(double* W169, double* V49, double* P0_169);  /* kiteEKF.cpp:6-13,26 */
int kite_nmpc_ekf_step(kite_nmpc_ctx* ctx, int32_t count, double dt, double* x13, const double* u3,
                       double* P169, const double* z7, const double* W169, const double* V49);
/* Same on device pointers, asynchronous on the context stream.              */
int kite_nmpc_ekf_step_device(kite_nmpc_ctx* ctx, int32_t count, double dt, double* d_x13,
                              const double* d_u3, double* d_P169, const double* d_z7,
                              const double* d_W169, const double* d_V49);

/* ---- wind-estimating EKF (build extension; additive, no version change) ---
 * The filter above with the world-frame wind W (m/s, a random walk) as three
 * more states: x16 = [x13 | W3], P256 count x 16 x 16 row-major, H = [0_{7x6}
 * I_7 0_{7x3}].  One call runs `substeps` propagations of dt / substeps (one
 * RK4 step of the wind model under the estimated wind, A = I + J h with
 * J = [df/dx | df/dW; 0], P = A P A' + W256) and, when z7 != NULL, one update
 * as kite_nmpc_ekf_step does it, after which P is made exactly symmetric
 * ((P + P') / 2: the update alone lets rounding asymmetry grow from period
 * to period).  x16 and P256 are updated in place; W256 /
 * V49 are shared by all kites.  status (count words, nullable) receives the
 * KITE_EKF_* bits, written (not OR-ed) on every call.  count < 1, dt <= 0 or
 * non-finite, substeps < 1 or > 2^24: KITE_EINVAL.                          */
#define KITE_EKF_NAN      1  /* estimate or P non-finite (on entry or in a substep):
                                the kite keeps its last finite x16 and P        */
#define KITE_EKF_S_NOT_PD 2  /* a pivot of S = H P H' + V was <= 0 or non-finite:
                                the update is skipped, the propagated estimate kept */
/* 13-state block and V: kite_ekf_default_covariances; wind block: 1e-4
 * (m/s)^2 per propagation on W256's diagonal, 25 (m/s)^2 on P0's.           */
void kite_windekf_default_covariances(double* W256, double* V49, double* P0_256);
int kite_nmpc_windekf_step(kite_nmpc_ctx* ctx, int32_t count, double dt, int32_t substeps, double* x16,
                           const double* u3, double* P256, const double* z7, const double* W256,
                           const double* V49, int32_t* status);
/* Same on device pointers, asynchronous on the context stream.              */
int kite_nmpc_windekf_step_device(kite_nmpc_ctx* ctx, int32_t count, double dt, int32_t substeps,
                                  double* d_x16, const double* d_u3, double* d_P256, const double* d_z7,
                                  const double* d_W256, const double* d_V49, int32_t* d_status);
/* The filter's Jacobian pass: J (count x 13 x 16, row-major) = [df/dx | df/dW]
 * of the wind model at (x13, u3) under the winds w3 (count x 3).            */
int kite_nmpc_jacobian_wind(kite_nmpc_ctx* ctx, int32_t count, const double* x13, const double* u3,
                            const double* w3, double* J);
/* kite_nmpc_set_wind from device memory, asynchronous on the context stream:
 * the B winds sit `stride` doubles apart at d_wind (stride >= 3; 16 when
 * d_wind points at column 13 of an x16 array).  Each component is clamped to
 * +-wmax and a non-finite one replaced by 0 (the device cannot refuse bad
 * values as the host entry does).  Switches the wind model on -- also for
 * all-zero winds -- and re-captures the step graph only when that switch
 * changes, not on a refresh of the values; kite_nmpc_set_wind(ctx, NULL)
 * returns to the reference model.  wmax <= 0 or non-finite, stride < 3:
 * KITE_EINVAL.                                                              */
int kite_nmpc_set_wind_device(kite_nmpc_ctx* ctx, const double* d_wind, int32_t stride, double wmax);

/* ---- kinematic (pose-only) EKF (build extension; additive, no version change)
 * The filter the reference's estimator node flies (ekf_node.cpp:235-241):
 * KiteEKF(Function, Function) (kiteEKF.cpp:54-72) over RigidBodyKinematics
 * (kite.cpp:622-661).  It has no aerodynamic model, no control and no
 * parameters: v_b and w_b are random walks, r' = vec(q (x) [0, v_b] (x)
 * conj(q)), q' = 1/2 q (x) [0, w_b] + 1/2 lambda q (q.q - 1) with lambda = -10,
 * and the 7 pose components are measured, H = [0_{7x6} I_7].  x13 (count x 13)
 * and P169 (count x 13 x 13, row-major) are updated in place; W169 / V49
 * (kite_ekf_default_covariances: the reference uses the same defaults in all
 * three constructors) are shared by all kites.  One call:
 *   with a frame:  z <- frame(z), on a copy (the caller's z7 is never written)
 *   with z7:       the copy's quaternion is negated when z_q . q_est < 0 at
 *                  entry (q and -q are one attitude; motion capture flips)
 *   `substeps` propagations of dt / substeps: A = I + J(x) h with the
 *                  closed-form J, one RK4 step, P = A P A' + W169
 *   with z7:       one update as kite_nmpc_windekf_step does it, then
 *                  P <- (P + P') / 2
 * Deviations from the reference: RK4 over the dt given (the reference's CVODES
 * integrates over a fixed 0.02 s whatever the filter's dt, kite.cpp:656-659
 * against kiteEKF.cpp:83-93); the quaternion sign alignment; the symmetrised P.
 * status (count words, nullable) receives KITE_EKF_NAN / KITE_EKF_S_NOT_PD,
 * written (not OR-ed) on every call, with kite_nmpc_windekf_step's meaning; a
 * non-finite measurement counts as a bad update (KITE_EKF_S_NOT_PD: the
 * propagated estimate is kept), not as a NaN kite.  count < 1, dt <= 0 or
 * non-finite, substeps < 1 or > 2^24, a zero-norm or non-finite frame
 * rotation: KITE_EINVAL.  kite_nmpc_set_estimator_model does not touch this
 * filter: it has no model.                                                   */
/* The motion-capture -> world change of a measured pose (optitrack2world,
 * ekf_node.cpp:148-169), z7 = (r, q):
 *   r <- r + vec(q (x) [0, offset] (x) conj(q))
 *   r <- vec(rotation (x) [0, r] (x) conj(rotation)) + shift
 *   q <- rotation (x) q (x) conj(rotation)
 * A NULL frame in the calls below means the poses are world poses already.   */
typedef struct { double offset[3]; double rotation[4]; double shift[3]; } kite_pose_frame;
/* the node's: offset (-0.09, 0, -0.02), rotation (0, -1, 0, 0), shift (0, 0, 2.77) */
void kite_pose_frame_default(kite_pose_frame* frame);
int kite_nmpc_kinekf_step(kite_nmpc_ctx* ctx, int32_t count, double dt, int32_t substeps, double* x13,
                          double* P169, const double* z7, const double* W169, const double* V49,
                          const kite_pose_frame* frame, int32_t* status);
/* Same on device pointers, asynchronous on the context stream; frame is a
 * host struct, passed by value into the launch.                             */
int kite_nmpc_kinekf_step_device(kite_nmpc_ctx* ctx, int32_t count, double dt, int32_t substeps,
                                 double* d_x13, double* d_P169, const double* d_z7, const double* d_W169,
                                 const double* d_V49, const kite_pose_frame* frame, int32_t* d_status);
/* The 13 states from two consecutive poses dt apart (KiteEKF_Node::initialize,
 * ekf_node.cpp:68-132), both through `frame` when one is given:
 *   rdot = (r_new - r_prev) / dt,  v_b = vec(conj(q_prev) (x) [0, rdot] (x) q_prev)
 *   dq = conj(q_prev) (x) q_new,   w_b = (2 / dt) vec(dq - [1, 0, 0, 0])
 *   x13 = [v_b, w_b, pose_new]
 * One deviation: q_new is negated for dq when q_prev . q_new < 0; the state
 * keeps pose_new as measured.  Per kite, dt <= 0 or non-finite or a
 * non-finite pose sets KITE_EKF_INIT_BAD in status (count words, nullable,
 * written on every call) and leaves that kite's x13 untouched; so dt is not
 * an argument error here.  count < 1 or a bad frame rotation: KITE_EINVAL.   */
#define KITE_EKF_INIT_BAD 4
int kite_nmpc_kinekf_init(kite_nmpc_ctx* ctx, int32_t count, double dt, const double* pose_prev7,
                          const double* pose_new7, const kite_pose_frame* frame, double* x13_out,
                          int32_t* status);
int kite_nmpc_kinekf_init_device(kite_nmpc_ctx* ctx, int32_t count, double dt, const double* d_pose_prev7,
                                 const double* d_pose_new7, const kite_pose_frame* frame, double* d_x13_out,
                                 int32_t* d_status);
/* The filter's Jacobian pass: J (count x 13 x 13, row-major) = df/dx of the
 * kinematic model at x13; rows 0..5 are zero.                                */
int kite_nmpc_jacobian_kin(kite_nmpc_ctx* ctx, int32_t count, const double* x13, double* J169);

/* ---- per-kite controller models (build extension; additive, no version change)
 * The model of the controller's predictions, per kite: the batch dimension
 * "one airframe per instance", and the way identified parameters
 * (kite_nmpc_identify_device) reach a running controller without leaving the
 * device.
 *   count == B     kite b's model is params[b]
 *   count == 1     one model for every kite (passed to the kernels as the
 *                  creation model is; also the form of a batch of one)
 *   params == NULL back to the creation model
 * Scope, as kite_nmpc_set_wind's: the model is used by every prediction of
 * kite_nmpc_step[_device] -- cold-start simulation, delay compensation,
 * sensitivities, defects -- with and without a controller wind, at every
 * horizon and with every qp_kernel.  The item-wise entry points (dynamics,
 * jacobian, predict, rk4_sens, colloc_eval, ident_*) and the plant's default
 * keep the creation model; so do both EKFs unless
 * kite_nmpc_set_estimator_model (below) hands them the controller's.  Rows
 * equal to the creation row give the creation model's outputs bit for bit.
 * A row must be a model (kite_nmpc_plant_set_params' rule: every field finite,
 * mass > 0, an invertible inertia, finite derived constants): one bad row is
 * KITE_EINVAL and the previous setting stays whole.  Any other count:
 * KITE_EINVAL.  count == B with cfg.sens_fp32 = 1 (and B > 1): KITE_ESTATE,
 * the fp32 sensitivity path holds one model.  The step graph is re-captured
 * when the call changes which kernels run or a model they hold by value
 * (count == 1, NULL, the first count == B), not when it refreshes the rows of
 * a per-kite setting.                                                        */
#define KITE_PARAMS_REJECTED 1   /* status bit: the row is no model, the kite keeps its previous one */
int kite_nmpc_set_params(kite_nmpc_ctx* ctx, const kite_params* params, int32_t count);
/* The count == B form from device memory (d_params52: B x 52 doubles, e.g. the
 * params_out of kite_nmpc_identify_device), asynchronous on the context
 * stream: one small kernel forms every kite's constants with the host's
 * arithmetic, bit for bit.  The device cannot refuse a row: a kite whose row
 * is no model keeps its previous one -- on the first call the model in force
 * until then, i.e. the creation model unless a count == 1 model was set --
 * and has KITE_PARAMS_REJECTED in d_status (B words, nullable, written on
 * every call, not OR-ed); the other kites are unaffected.  count != B or a
 * NULL row pointer: KITE_EINVAL; cfg.sens_fp32 = 1: KITE_ESTATE.  Only the
 * first call (the switch to per-kite kernels) re-captures the step graph.    */
int kite_nmpc_set_params_device(kite_nmpc_ctx* ctx, const double* d_params52, int32_t count, int32_t* d_status);
/* The B rows in force (host pointer, B x kite_params): what the setters above
 * left, the creation row B times when none was called.  Waits for the context
 * stream when a per-kite setting is in force.                                 */
int kite_nmpc_get_params(kite_nmpc_ctx* ctx, kite_params* out);
/* The model of the two estimators (kite_nmpc_ekf_step[_device],
 * kite_nmpc_windekf_step[_device]).  KITE_EST_MODEL_CREATION: the creation
 * model whatever the controller's setting, as every context starts.
 * KITE_EST_MODEL_CONTROLLER: the controller's models in force at the call --
 *   the creation model (no kite_nmpc_set_params, or NULL): as with mode 0;
 *   one model (the count == 1 form): that model, for any `count`;
 *   a model per kite: kite b of the call filters with the row in force of
 *     kite b, so `count` must be the context's B (anything else: KITE_EINVAL,
 *     nothing is launched, x and P stay); a kite whose row the device setter
 *     rejected filters with the row it kept.
 * Ordering is the stream's: a filter call issued after
 * kite_nmpc_set_params_device sees the new rows without synchronisation.
 * Rows equal to the creation row give the creation model's estimates bit for
 * bit.  The item-wise entry points (kite_nmpc_jacobian_wind among them) keep
 * the creation model.  The kinematic filter (kite_nmpc_kinekf_step[_device])
 * is not touched: it has no model.  Any other mode: KITE_EINVAL.             */
#define KITE_EST_MODEL_CREATION   0
#define KITE_EST_MODEL_CONTROLLER 1
int kite_nmpc_set_estimator_model(kite_nmpc_ctx* ctx, int32_t mode);
int kite_nmpc_get_estimator_model(kite_nmpc_ctx* ctx, int32_t* mode);

/* ---- two-phase tiled QP (additive, no version change) ----------------------
 * At N = 20 with the tiled QP (qp_kernel 2) the main solve can run in two
 * launches: the first stops every kite that has not converged at the top of
 * interior-point iteration `split_iteration` (a constant of the build), the
 * second resumes them from a checkpoint, dispatched by their residual at that
 * point, largest first -- the waves of a large batch queue per SIMD, and this
 * order shortens the tail of the launch.  Every kite's result is bit for bit
 * the one-launch solve's.
 *   KITE_QP_SPLIT_AUTO   (default) split when the batch is large enough for
 *                        several waves to queue per SIMD on this device
 *   KITE_QP_SPLIT_NEVER  one launch
 *   mode > 0             split at any batch
 * Any other horizon or qp_kernel: accepted and without effect.  mode < -1:
 * KITE_EINVAL.  The getter's outputs are each nullable: the mode set, whether
 * the next step splits (1 / 0), the build's split iteration, and how many
 * launch sequences have been issued with the split since creation (a step
 * replayed from a captured graph counts once, at its capture).               */
#define KITE_QP_SPLIT_AUTO  (-1)
#define KITE_QP_SPLIT_NEVER 0
int kite_nmpc_set_qp_split(kite_nmpc_ctx* ctx, int32_t mode);
int kite_nmpc_get_qp_split(kite_nmpc_ctx* ctx, int32_t* mode, int32_t* active, int32_t* split_iteration,
                           int64_t* split_launches);

/* ---- aerodynamic parameter identification (additive, no version change) ----
 * src/kite_control/kite_identification_test.cpp: fit the 21 aerodynamic
 * coefficients of a kite to a logged flight, batched over `count` kites.
 * Identified parameters (the reference's REF_P order, :120-121), as
 * kite_params fields:
 *   CL0 CLa_total CD0_total CYb Cm0 Cma Cnb Clb CLq Cmq CYr Cnr Clr CYp Clp
 *   Cnp CLde CYdr Cmde Cndr Cldr
 * everything else of a kite's kite_params row is a known constant of that kite.
 * Log per kite: X (T+1) x 13, U T x 3 (T, dE, dR), sample interval h.
 *   model      RK4, `substeps` substeps of h / substeps under the held control,
 *              no wind (the plant's integrator); the _wind entries below take a
 *              logged wind
 *   segments   the log is cut into segments of `segment` = L samples; a segment
 *              starts at the measured X[k0] with zero sensitivity and predicts
 *              x^_{k0+1} .. x^_{k0+L} (the last one may be shorter).  L = 1: the
 *              one-step prediction error; L = T: single shooting
 *   variables  z_j = (p_j - pref_j) / s_j, s_j = |pref_j| (1 where that is 0),
 *              pref the kite's input row
 *   cost       c = 1/T sum_k e_k' Q e_k + alpha |z|^2,  e_k = X[k] - x^_k
 *   normal eq. A = 1/T sum S~' Q S~ + alpha I,  g = 1/T sum S~' Q e - alpha z,
 *              S~ = (d x^_k / d p) diag(s)
 *   box        -lb_rel <= z <= ub_rel (+INFINITY: that side is free)
 * Iteration (per kite, `iters` evaluations, all on the device): evaluate c, A,
 * g at the trial; accept it when c is finite and not above the accepted cost
 * (lambda /= 4, floor 1e-12), else reject (lambda *= 8, cap 1e6); active set =
 * variables on a bound whose gradient points outward; solve
 * (A + lambda tr(A)/21 I) s = g on the free variables (Cholesky; a pivot <= 0 or
 * non-finite: s = 0, lambda *= 8); trial = clip(z + s); an accepted evaluation
 * with |s|_inf < tol ends the kite (KITE_IDENT_CONVERGED).  The result is the
 * last accepted point: always an evaluated one, its cost never above the first. */
#define KITE_IDENT_NP        21
#define KITE_IDENT_CHUNK      8  /* samples per partial sum of the accumulation kernel
                                    (whole segments: max(1, 8 / L) segments of L)    */
#define KITE_IDENT_NAN        1  /* log or parameter row non-finite (or not a model), or
                                    no evaluation was finite: the input row is returned */
#define KITE_IDENT_CONVERGED  2
#define KITE_IDENT_AT_BOUND   4  /* some identified parameter ends on its box        */
typedef struct kite_ident_config {
    int32_t substeps;     /* RK4 substeps per sample interval, 1..64 (4)             */
    int32_t segment;      /* L, samples per segment, 1..T (1)                        */
    int32_t iters;        /* evaluations, 1..64 (12)                                 */
    int32_t reserved;
    double h;             /* sample interval [s] (0.02)                              */
    double Q[13];         /* per-state weight (kite_identification_test.cpp:193)     */
    double alpha;         /* weight of |z|^2 (0; the reference's fitting_error2: 100) */
    double lm0;           /* initial lambda (1e-6)                                   */
    double tol;           /* convergence: |s|_inf of an accepted evaluation (1e-10)  */
    double lb_rel[21], ub_rel[21];   /* box of z (:127-148)                          */
} kite_ident_config;
void kite_ident_default_config(kite_ident_config* cfg);
/* kite_params field index (0..51) of identified parameter j, -1 outside 0..20. */
int kite_ident_param_index(int32_t j);
/* Building block: one sample interval per item.  x13_out (count x 13) and
 * S = d x+ / d p (count x 13 x 21, unscaled) after `substeps` RK4 substeps of
 * h / substeps.  params: nparams rows, nparams == 1 (one row for all) or count;
 * a row that is no model (kite_nmpc_plant_set_params' rule): KITE_EINVAL.     */
int kite_nmpc_ident_sens(kite_nmpc_ctx* ctx, int32_t count, double h, int32_t substeps,
                         const kite_params* params, int32_t nparams, const double* x13, const double* u3,
                         double* x13_out, double* S);
/* One evaluation at p21 (count x 21 parameter values): A (count x 21 x 21, full,
 * exactly symmetric), g (count x 21), cost (count) in the scaled variables;
 * status (count, nullable): KITE_IDENT_NAN where the cost is not finite.
 * cfg->iters, lm0, tol and the box are not used.                              */
int kite_nmpc_ident_normal(kite_nmpc_ctx* ctx, const kite_ident_config* cfg, int32_t count, int32_t T,
                           const kite_params* params, int32_t nparams, const double* p21, const double* X,
                           const double* U, double* A, double* g, double* cost, int32_t* status);
/* The identification.  params_out count x 52 (the input row with the 21
 * replaced), cost2 count x 2 (first and final accepted cost), evals count
 * (evaluations done), status count (KITE_IDENT_* bits, written on every call);
 * the last three are nullable.  A row with a non-finite field is contained
 * (KITE_IDENT_NAN, the other kites are not affected); a finite row that is no
 * model is KITE_EINVAL.  T < 1, T > 2^20, substeps outside 1..64, segment
 * outside 1..T, iters outside 1..64, h <= 0 or non-finite, a negative or
 * non-finite Q / alpha / lm0 / tol, a negative or NaN lb_rel / ub_rel:
 * KITE_EINVAL, nothing is launched.  count is free of the context's batch.   */
int kite_nmpc_identify(kite_nmpc_ctx* ctx, const kite_ident_config* cfg, int32_t count, int32_t T,
                       const kite_params* params, int32_t nparams, const double* X, const double* U,
                       kite_params* params_out, double* cost2, int32_t* evals, int32_t* status);
/* Same on device pointers (d_params: nparams x 52 doubles) with a workspace of
 * kite_nmpc_ident_workspace_doubles doubles: 2 * iters launches on the context
 * stream, no allocation, no copy, no synchronisation.  The device cannot refuse
 * a row: one that is no model is KITE_IDENT_NAN.                              */
int kite_nmpc_identify_device(kite_nmpc_ctx* ctx, const kite_ident_config* cfg, int32_t count, int32_t T,
                              const double* d_params, int32_t nparams, const double* d_X, const double* d_U,
                              double* d_params_out, double* d_cost2, int32_t* d_evals, int32_t* d_status,
                              double* d_workspace);
/* Workspace of the device variant in doubles; KITE_EINVAL (negative) for
 * arguments kite_nmpc_identify refuses.                                       */
int64_t kite_nmpc_ident_workspace_doubles(const kite_ident_config* cfg, int32_t count, int32_t T);
/* ---- the identification under a logged wind (additive, no version change) ----
 * The same fit with a KNOWN world-frame wind per sample [m/s]: the model's
 * aerodynamics see v_a = v - q^-1 (x) [0,W] (x) q (kite_nmpc_set_wind's
 * model), gravity, tether and kinematics keep v.  The unknowns stay the 21;
 * formulation, iteration rule, chunking, slab and workspace
 * (kite_nmpc_ident_workspace_doubles serves both forms) are those above.
 * Wind log per kite: W T x 3, row k held over sample interval k exactly as
 * U[k] is; a constant wind is a log of equal rows.  Where it comes from is the
 * caller's business: a wind known for a sweep, or the wind EKF's estimate
 * (kite_nmpc_windekf_step).  The plant's gust (kite_nmpc_plant_set_wind) varies
 * inside a sample while the log holds one value per sample: a log of a gusting
 * plant is an approximation, a constant wind is exact.
 * The argument rules are those of the windless entries.  A NULL wind pointer
 * runs the windless kernels and is bit for bit the windless entry.  A
 * non-finite wind entry makes that kite's cost non-finite: the kite returns its
 * input row with KITE_IDENT_NAN, the others are not affected.
 * kite_nmpc_ident_sens_wind: w3 count x 3, the item's wind.                    */
int kite_nmpc_ident_sens_wind(kite_nmpc_ctx* ctx, int32_t count, double h, int32_t substeps,
                              const kite_params* params, int32_t nparams, const double* x13, const double* u3,
                              const double* w3, double* x13_out, double* S);
/* W: count x T x 3. */
int kite_nmpc_ident_normal_wind(kite_nmpc_ctx* ctx, const kite_ident_config* cfg, int32_t count, int32_t T,
                                const kite_params* params, int32_t nparams, const double* p21, const double* X,
                                const double* U, const double* W, double* A, double* g, double* cost,
                                int32_t* status);
int kite_nmpc_identify_wind(kite_nmpc_ctx* ctx, const kite_ident_config* cfg, int32_t count, int32_t T,
                            const kite_params* params, int32_t nparams, const double* X, const double* U,
                            const double* W, kite_params* params_out, double* cost2, int32_t* evals,
                            int32_t* status);
/* d_W: count x T x 3 on the device, read by every one of the 2 * iters launches. */
int kite_nmpc_identify_wind_device(kite_nmpc_ctx* ctx, const kite_ident_config* cfg, int32_t count, int32_t T,
                                   const double* d_params, int32_t nparams, const double* d_X, const double* d_U,
                                   const double* d_W, double* d_params_out, double* d_cost2, int32_t* d_evals,
                                   int32_t* d_status, double* d_workspace);
/* ---- the wind identified jointly with the 21 (additive, no version change) ----
 * For a fleet whose wind nobody knows: per kite and log, 24 unknowns.
 *   unknowns   the 21 coefficients and a constant world-frame wind offset w (3)
 *   model      the model of sample k sees the wind W0[k] + w (the logged-wind
 *              model above).  W0 is an optional known log, count x T x 3, NULL =
 *              zeros: NULL is "no idea of the wind", W0 = a logged estimate (the
 *              wind EKF's) is "correct the bias of that estimate"
 *   variables  z[0:21] as above; z[21:24] = (w - w_prior) / w_scale
 *   cost       c = 1/T sum_k e_k' Q e_k + alpha |z[0:21]|^2 + alpha_w |z[21:24]|^2
 *   normal eq. A = 1/T sum S~' Q S~ + diag(alpha I21, alpha_w I3),
 *              g = 1/T sum S~' Q e - (alpha z[0:21], alpha_w z[21:24]),
 *              S~ = (d x^_k / d (p, w)) diag(s, w_scale), 13 x 24
 *   box        the 21 as above; |w_i - w_prior_i| <= w_box_i (+INFINITY = free)
 * Segments, chunking (KITE_IDENT_CHUNK), the ordered atomics-free sums and the
 * iteration rule are those of the 21: accept / reject, lambda /4 and x8, active
 * set, Cholesky on the free set, clip, tol -- with 24 variables, and the damping
 * lambda tr(A) / 24.  The iteration starts at the input row and w = w_prior.
 * Status: the bits above keep their meaning (KITE_IDENT_AT_BOUND: one of the 21
 * ends on its box); KITE_IDENT_WIND_AT_BOUND: a wind component ends on its box.
 * A non-finite entry in W0, the log or the row makes that kite's cost
 * non-finite, which is never accepted: the kite returns its input row and
 * w_prior with KITE_IDENT_NAN, the others are not affected.
 * Argument rules: those of the _wind entries; in addition w_scale <= 0 or
 * non-finite, a negative or NaN w_box / alpha_w (alpha_w also non-finite), a
 * non-finite w_prior, or a NULL wind config: KITE_EINVAL, nothing is launched. */
#define KITE_IDENT_NPW       24  /* the 21 and the wind offset                       */
#define KITE_IDENT_WIND_AT_BOUND 8
typedef struct kite_ident_wind_config {
    double w_scale;       /* scale of the wind variables [m/s] (1.0)                 */
    double w_prior[3];    /* centre of the box, start of the iteration [m/s] (0)     */
    double w_box[3];      /* half-width of the box [m/s] (3.0; +INFINITY: free)      */
    double alpha_w;       /* weight of |z[21:24]|^2 (0)                              */
} kite_ident_wind_config;
void kite_ident_wind_default_config(kite_ident_wind_config* cfg);
/* One sample interval per item under the wind w3 (count x 3, the total wind):
 * x13_out and S = d x+ / d (p, w), count x 13 x 24, unscaled.                 */
int kite_nmpc_ident_sens_joint(kite_nmpc_ctx* ctx, int32_t count, double h, int32_t substeps,
                               const kite_params* params, int32_t nparams, const double* x13, const double* u3,
                               const double* w3, double* x13_out, double* S);
/* One evaluation at p21 (count x 21) and the wind offset w3 (count x 3): A
 * (count x 24 x 24, full, exactly symmetric), g (count x 24), cost (count);
 * W0 count x T x 3 or NULL.  iters, lm0, tol and the boxes are not used.      */
int kite_nmpc_ident_normal_joint(kite_nmpc_ctx* ctx, const kite_ident_config* cfg,
                                 const kite_ident_wind_config* wcfg, int32_t count, int32_t T,
                                 const kite_params* params, int32_t nparams, const double* p21, const double* w3,
                                 const double* X, const double* U, const double* W0, double* A, double* g,
                                 double* cost, int32_t* status);
/* The joint identification.  params_out count x 52, wind_out count x 3 (the
 * identified offset w; the model's wind is W0 + w), cost2, evals, status as
 * kite_nmpc_identify.                                                          */
int kite_nmpc_identify_joint(kite_nmpc_ctx* ctx, const kite_ident_config* cfg, const kite_ident_wind_config* wcfg,
                             int32_t count, int32_t T, const kite_params* params, int32_t nparams, const double* X,
                             const double* U, const double* W0, kite_params* params_out, double* wind_out,
                             double* cost2, int32_t* evals, int32_t* status);
/* Same on device pointers with a workspace of
 * kite_nmpc_ident_joint_workspace_doubles doubles: 2 * iters launches on the
 * context stream, no allocation, no copy, no synchronisation.  d_W0 nullable. */
int kite_nmpc_identify_joint_device(kite_nmpc_ctx* ctx, const kite_ident_config* cfg,
                                    const kite_ident_wind_config* wcfg, int32_t count, int32_t T,
                                    const double* d_params, int32_t nparams, const double* d_X, const double* d_U,
                                    const double* d_W0, double* d_params_out, double* d_wind_out, double* d_cost2,
                                    int32_t* d_evals, int32_t* d_status, double* d_workspace);
int64_t kite_nmpc_ident_joint_workspace_doubles(const kite_ident_config* cfg, int32_t count, int32_t T);

/* Per-kernel device time [ms] of the last step (cfg.timing = 1):
 * [prologue, rk4_sens, condense, qp, total, qp_main]; qp is the whole QP
 * phase (solve, expansion, lazy state rows), qp_main the main QP kernel
 * alone (k_qp_tiled / k_qp_lds / k_qp / k_qp_ric: the roofline's kernel).
 * Returns the entries written, min(n, 6).                                   */
int kite_nmpc_kernel_times(kite_nmpc_ctx* ctx, double* ms, int32_t n);
/* Time every kernel of the next max_steps steps with a ring of HIP events
 * (no host synchronisation between steps); timing_read waits for the last
 * recorded step and returns the number of steps recorded, with per-kernel
 * SUMS [ms] in the first min(n, 6) entries of sums_ms:
 * [prologue, rk4_sens, condense, qp, total, qp_main] (as kernel_times).   */
int kite_nmpc_timing_start(kite_nmpc_ctx* ctx, int32_t max_steps);
/* The same ring, recording only every stride-th step from the next one on
 * (steps 0, stride, 2 stride, ...), at most max_samples of them; timing_read
 * returns the number recorded.  Each recorded step places six events between
 * its kernels (~4.6 us each on gfx950); sampling keeps that measurement cost
 * out of the other steps of a timed run.  stride 1 = kite_nmpc_timing_start
 * (since API 7).                                                           */
int kite_nmpc_timing_start_sampled(kite_nmpc_ctx* ctx, int32_t max_samples, int32_t stride);
int kite_nmpc_timing_read(kite_nmpc_ctx* ctx, double* sums_ms, int32_t n);
/* QP statistics of the last step: final residual and interior-point
 * iterations per instance (host pointers, B each; either may be NULL).    */
int kite_nmpc_qp_stats(kite_nmpc_ctx* ctx, double* kkt, int32_t* iters);
/* Interior-point iterations summed over all instances and all steps since
 * the last kite_nmpc_timing_start (or since create): the measurement hook
 * behind bench.py's FLOP count (no reference counterpart).                */
int kite_nmpc_qp_iteration_sum(kite_nmpc_ctx* ctx, int64_t* sum);
/* State-box enforcement since the last kite_nmpc_timing_start (or since
 * create), summed over instances and steps: kite-steps whose committed plan
 * leaves the state box (status bit 8) and the (node, state) pairs outside it
 * (states 1..12, nodes 1..N, tolerance 1e-8 max(1, |bound|)); with the
 * multiple-shooting QP the latter are the soft rows with xi > 0 at the
 * accepted solution.  The reference's NLP holds these as hard bounds
 * (kiteNMPF.cpp:154-167); measurement hook, either pointer may be NULL.    */
int kite_nmpc_state_bound_stats(kite_nmpc_ctx* ctx, int64_t* steps_outside, int64_t* rows_outside);
/* Condensed QP of one instance from the last step (scaled variables, GPU
 * column order: [T,dE,dR]_k (3N) | Uv_k (N) | theta0 | thetadot0).
 * H n x n, h n, C N x n, cl/cu N (+-INF = absent), n = 4N+2.               */
int kite_nmpc_get_qp(kite_nmpc_ctx* ctx, int32_t instance, double* H, double* h,
                     double* C, double* cl, double* cu);
int kite_nmpc_batch(const kite_nmpc_ctx* ctx);
int kite_nmpc_api_version(void);

/* ---- closed-loop scoring (score_kernels.hip; no reference counterpart) ----
 * What a flown episode is judged by, kept on the device: one launch per
 * control period reads the true kite state and the control applied and adds
 * the period to a row of fp64 accumulators per kite; a second kernel reduces
 * the rows to a fleet summary.  The path, Q, R, Sx and Su are the context's
 * configuration; `count` need not be the context's batch.  Additive to API 7.
 *
 * The distance is the true cross-track error: the distance to the GLOBAL
 * closest point of the path (64 samples of theta, then a safeguarded Newton
 * iteration clamped to the best sample's neighbours), not the distance to the
 * plan's virtual theta0 (kite_mpc_diagnostic.pos_error) and not the local
 * warm-start search of kite_nmpc_closest_point.                              */
#define KITE_SCORE_NACC 16   /* doubles per kite in acc  */
#define KITE_SCORE_NSUM 16   /* doubles of the summary   */
#define KITE_SCORE_NMEM 8    /* doubles per kite in mem  */
/* acc row of one kite; all zero = reset.  Slots 0-2 and 11-14 hold integers. */
#define KITE_SCORE_N              0   /* scored periods                                          */
#define KITE_SCORE_N_LOST         1   /* lost periods                                            */
#define KITE_SCORE_EVER_LOST      2   /* 1 once a period was lost                                */
#define KITE_SCORE_SUM_D2         3   /* sum d^2 [m^2], d = ||P(theta*) - r||                     */
#define KITE_SCORE_MAX_D          4   /* max d [m] (meaningful when N > 0)                       */
#define KITE_SCORE_SUM_TRACK      5   /* sum_a Q_a (Sx[6+a] (P(theta*) - r)_a)^2, summed          */
#define KITE_SCORE_SUM_U          6   /* sum_i R_i (Su_i u_i)^2, summed                          */
#define KITE_SCORE_SUM_RATE       7   /* ||Su (u - u_prev)||^2, summed over N_RATE periods       */
#define KITE_SCORE_SUM_SPEED      8   /* sum ||v_b|| [m/s]                                       */
#define KITE_SCORE_MIN_SPEED      9   /* min ||v_b|| [m/s] (meaningful when N > 0)               */
#define KITE_SCORE_PROGRESS      10   /* sum wrap(theta* - theta*_prev) [rad], wrap to (-pi, pi];
                                         laps = progress / 2 pi                                  */
#define KITE_SCORE_N_MIN_SPEED   11   /* scored periods with KITE_ST_MIN_SPEED                   */
#define KITE_SCORE_N_QP_NOT_CONV 12   /* scored periods with KITE_ST_QP_NOT_CONV                 */
#define KITE_SCORE_N_STATE_BOUND 13   /* scored periods with KITE_ST_STATE_BOUND                 */
#define KITE_SCORE_N_RATE        14   /* periods that added to SUM_RATE and PROGRESS             */
#define KITE_SCORE_SPARE         15   /* 0                                                       */
/* The summary holds the same slots over the kites as RAW values: sums, except
 * the max of MAX_D and the min of MIN_SPEED (over the kites with N > 0; 0 when
 * there is none), and in slot 15 the number of rows reduced.  Summaries of
 * shards therefore combine by +, max and min (a shard with N = 0 has no max
 * and no min).                                                               */
#define KITE_SCORE_KITES         15
/* mem row of one kite; all zero = reset */
#define KITE_SCORE_MEM_THETA      0   /* theta* of the last scored period                        */
#define KITE_SCORE_MEM_U          1   /* u4 of the last scored period (slots 1-4)                */
#define KITE_SCORE_MEM_VALID      5   /* 1: slots 0-4 are the period before this one             */
                                      /* slots 6, 7: spare                                       */

/* theta* in [-2 pi / 64, 2 pi) and d = ||P(theta*) - pos|| of the global closest
 * point for `count` positions (count x 3).  A non-finite position gives NaN
 * in both.  Host pointers; _device: device pointers, asynchronous on the
 * context's stream.                                                          */
int kite_nmpc_closest_point_global(kite_nmpc_ctx* ctx, int32_t count, const double* pos3,
                                   double* theta_out, double* dist_out);
int kite_nmpc_closest_point_global_device(kite_nmpc_ctx* ctx, int32_t count, const double* d_pos3,
                                          double* d_theta_out, double* d_dist_out);
/* Score one control period of `count` kites: x13 (count x 13) the true state at
 * t0, u4 (count x 4) the control applied from t0, status the controller's
 * status words and plant_status the plant's (count each, either may be NULL),
 * first != 0 at the start of an episode (no rate and no progress against the
 * period before).  acc (count x 16) and mem (count x 8) are updated in place.
 * A period is LOST when the plant status has KITE_PLANT_NAN, x13 or u4 is
 * non-finite (or so large that a scored quantity overflows), or the
 * controller status has KITE_ST_NAN, KITE_ST_STEP_REJECTED or
 * KITE_ST_RESTART: it adds 1 to N_LOST, sets EVER_LOST, clears MEM_VALID (the
 * next period adds no rate and no progress) and touches nothing else.  Any
 * other period is scored into the slots above, with plain fp64 additions in
 * call order; a kite's row depends on its own inputs only.                  */
int kite_nmpc_score_step(kite_nmpc_ctx* ctx, int32_t count, const double* x13, const double* u4,
                         const int32_t* status, const int32_t* plant_status, int32_t first,
                         double* acc, double* mem);
int kite_nmpc_score_step_device(kite_nmpc_ctx* ctx, int32_t count, const double* d_x13, const double* d_u4,
                                const int32_t* d_status, const int32_t* d_plant_status, int32_t first,
                                double* d_acc, double* d_mem);
/* out16 (KITE_SCORE_NSUM) from acc (count x 16), in a fixed order without
 * atomics: two calls on the same acc agree bit for bit.                     */
int kite_nmpc_score_summary(kite_nmpc_ctx* ctx, int32_t count, const double* acc, double* out16);
int kite_nmpc_score_summary_device(kite_nmpc_ctx* ctx, int32_t count, const double* d_acc, double* d_out16);

#ifdef __cplusplus
}
#endif
#endif /* KITE_NMPC_H */
