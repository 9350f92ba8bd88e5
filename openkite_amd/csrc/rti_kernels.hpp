// rti_kernels.hpp -- internal interface between the C ABI (kite_nmpc.cpp) and
// the gfx950 kernels (rti_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kite_model.hpp"
#include "kite_path.hpp"

// Largest horizon the fused condense/QP kernels are built for (LDS budget of
// the wave-per-instance QP).  n = 4N+2 <= 82 decision variables.
#define KITE_NMAX 40

namespace kite {

// Everything the RTI kernels need besides the model, precomputed on the host
// from kite_nmpc_config (kernel argument, < 1 KiB).
struct RtiConst {
    int N, M, K, n;
    int shift, lo_fin, hi_fin, pad_;
    double dt, h;
    double sqQ_dt[3];   // sqrt(dt Q_i)   stage path weights
    double sqQ_T[3];    // sqrt(Q_i)      Mayer path weights (kiteNMPF.cpp:141)
    double sw;          // sqrt(dt W)
    double Sr[3];       // Sx[6..8]
    double sv;          // Sx[14]
    double vref;        // physical
    double Rdiag[4];    // dt R_c Su_c^2
    double Rraw[4];     // R_c
    double Su[4], Sx13, Sx14;
    double lbx[15], ubx[15], lbu[4], ubu[4];
    double flex, min_speed;
    double path_R, path_alt, pq[4];
    double delay;       // delay compensation [s] (0 = off)
    int delay_steps, delay_node;
    int sens_fp32, pad2_;   // 1: k_rk4_sens2 in fp32 (DualF2)
    int path_K, pad3_;      // 0: circle (path_R, path_alt); 1..8: Fourier path pF (kite_path.hpp)
    double pF[3][KITE_PATH_NC];
};

// Start multiplier z0 of the multiple-shooting IPM (qp_ric.inc; the oracle's
// MS_Z0 holds the same value).  A soft state row starts dual feasible only if
// its weight exceeds 2 z0 (z2 = soft_w - z0 > z0): kite_nmpc_create /
// set_bounds refuse qp_soft_weight <= RIC_SOFT_WEIGHT_MIN for qp_kernel 3.
constexpr double RIC_Z0 = 20.0;
constexpr double RIC_SOFT_WEIGHT_MIN = 2.0 * RIC_Z0;

// Multiple-shooting QP + Riccati interior point (qp_ric.inc, oracle qp_form 1):
// constants precomputed on the host from kite_nmpc_config.
struct RicConst {
    double soft_w;      // L1 weight of the soft state bounds (scaled units)
    double lm;          // Levenberg-Marquardt term on every QP variable
    double hth, g0, g1; // scaled theta dynamics: th' = th + hth thd + g0 Uv, thd' = thd + g1 Uv
    double sq[2][3];    // path rows sqrt(w Q_a): [0] k < N (w = dt), [1] k = N (w = 1)
    double sw;          // speed row sqrt(dt W)
    double ctheta;      // Sx[6+a] / Sx13 factor of dP/dtheta in the theta column: 1 / Sx13
    double Rh[4];       // control Hessian (scaled): dt R_c
    double lb[20], ub[20], sc[20];   // per stage slot: bound and scale (see qp_ric.inc)
    int nC;             // complementarity pairs per kite (rows + soft rows over all stages)
    int lomask[3], himask[3];        // bit j: slot j has a lower / upper bound row at stage
                                     // type t (0: k = 0, 1: 0 < k < N, 2: k = N)
    int nb[3];                       // bounded slots per stage type ...
    int8_t bslot[3][20];             // ... and their slot numbers
};
bool qp_ric_supported(const RtiConst& C);
size_t qp_ric_lds_bytes(const RtiConst& C, const RicConst& R);
// C, R: host copies (launch geometry); Cd, Rd: the same constants in device memory;
// ws: workspace of qp_ric_ws_doubles(C) doubles per kite
size_t qp_ric_ws_doubles(const RtiConst& C);
hipError_t launch_qp_ric(const RtiConst& C, const RicConst& R, const RtiConst* Cd, const RicConst* Rd, int B,
                         const double* AB, const double* DEF, double* X, double* U, double* u0, double* diag,
                         int32_t* status, double* kkt, int32_t* iters, int32_t* iters_acc, const int32_t* order,
                         double* ws, hipStream_t s, hipEvent_t after_main = nullptr);

// wind: per-kite constant world-frame wind (B x 3, m/s) or nullptr (the
// reference model, no wind; kite_model.hpp kite_rhs<T, WIND>)
// cold: B + 1 ints, the prologue's cold-restart list (count first; zero on
// entry -- k_qp_order empties it every step)
// mct: per-kite model constants, kite-major [B][kModelTableStride] doubles (a
// kite's ModelConst and a pad), or nullptr: every kite takes P (kernel
// argument).  With a table the sensitivities are fp64 only (C.sens_fp32 == 0).
// sched: the in-flight schedule, B x KITE_INFLIGHT_N (launch_inflight), or
// nullptr: the delay compensation predicts under the previous u(t0)
hipError_t launch_prologue(const ModelConst& P, const RtiConst& C, int B, int warm, const double* x0,
                           double* X, double* U, int32_t* status, const double* wind, int32_t* cold,
                           const double* mct, const double* sched, hipStream_t s);
// sched (B x KITE_INFLIGHT_N) <- the schedule rows of the lines (B x
// KITE_DELAY_NLINE) seen at time t0 (k_inflight; delay_line.hpp)
hipError_t launch_inflight(int B, const double* line, double t0, double* sched, hipStream_t s);
hipError_t launch_rk4_sens(const ModelConst& P, const RtiConst& C, int B, const double* X, const double* U,
                           double* AB, double* DEF, const double* wind, const double* mct, hipStream_t s);
constexpr int kModelTableStride = 48;
// Kite b's table row as a ModelConst, for kernels in which b is wave-uniform
// (a wave is one kite): the row address is uniform and the row arrives by
// scalar loads into the SGPRs that hold the kernel-argument ModelConst of the
// homogeneous kernels.
__device__ __forceinline__ ModelConst model_row(const double* __restrict__ mct, int b) {
    const double* r = mct + (size_t)b * kModelTableStride;
    ModelConst P;
    double* g = reinterpret_cast<double*>(&P);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(ModelConst) / sizeof(double)); ++i) g[i] = r[i];
    return P;
}
// every row of the table mct and of the rows in force (rows, B x 52) from one
// model: its constants P and its kite_params row52 (host pointer)
hipError_t launch_model_fill(const ModelConst& P, const double* row52, int B, double* mct, double* rows,
                             hipStream_t s);
// the table from B kite_params rows in device memory (k_model_const): a row
// that is a model replaces the kite's table row and row in force, any other
// keeps both; status: B words (nullable), KITE_PARAMS_REJECTED per kite,
// written on every call.  d_rows52 may be `rows` itself.
hipError_t launch_model_const(int B, const double* d_rows52, double* mct, double* rows, int32_t* status,
                              hipStream_t s);
hipError_t launch_condense(const RtiConst& C, int B, const double* X, const double* U, const double* AB,
                           const double* DEF, double* Hs, double* hs, double* Cr, double* cl, double* cu,
                           double* hmax, int tiled, double* Htl, double* Hab, double* Hbb, hipStream_t s);
// Tiled-QP path (N == 20): H_aa as 15 lower 16x16 C-layout tiles in lane order.
bool qp_tiled_supported(const RtiConst& C);
// split (N == 20 only, nullptr: the solve in one launch): the main solve in
// two launches, the second dispatched by a key from inside the solve
// (qp_tiled.inc).  ckpt: B x qp_split_ckpt_doubles() doubles, key and order2: B
// words each.  after_main then follows the second launch.
struct QpSplitBufs {
    double* ckpt;
    int32_t* key;
    int32_t* order2;
};
size_t qp_split_ckpt_doubles();
int qp_split_iteration();          // the build's QP_SPLIT_IT
hipError_t launch_qp_tiled(const ModelConst& P, const RtiConst& C, int B, const double* Htl, const double* Hab,
                           const double* Hbb, const double* hs, const double* Cr, const double* cl,
                           const double* cu, const double* hmax, const double* AB, const double* DEF, double* X,
                           double* U, double* u0, double* diag, int32_t* status, double* kkt, int32_t* iters,
                           const int32_t* order, int32_t* lazy, double* wstep, hipStream_t s,
                           hipEvent_t after_main = nullptr, const QpSplitBufs* split = nullptr);
hipError_t launch_qp(const ModelConst& P, const RtiConst& C, int B, const double* Hs, const double* hs,
                     const double* Cr, const double* cl, const double* cu, const double* hmax,
                     const double* AB, const double* DEF, double* X, double* U, double* u0, double* diag,
                     int32_t* status, double* kkt, int32_t* iters, const int32_t* order, int32_t* lazy,
                     hipStream_t s, hipEvent_t after_main = nullptr);
// QP grid dispatch order: kites by the previous step's iteration count, most
// first; also empties the lazy state-bound list (lazy[0] = 0, B + 1 entries)
// and the prologue's cold list that follows it (lazy[B + 1] = 0)
hipError_t launch_publish(int B, int N, const double* u0, const double* X, const double* U, const double* diag,
                          const int32_t* status, double* d_u0, double* d_traj, double* d_ctrl, double* d_diag,
                          int32_t* d_status, hipStream_t s);
hipError_t launch_qp_order(const RtiConst& C, int B, const int32_t* iters, int32_t* order, int32_t* lazy,
                           hipStream_t s);
// the same sort over keys in [0, max_key] (max_key <= 255), largest first,
// without touching either list
hipError_t launch_qp_order_keys(int B, int max_key, const int32_t* keys, int32_t* order, hipStream_t s);
hipError_t launch_dynamics(const ModelConst& P, int count, const double* x, const double* u, double* f,
                           hipStream_t s);
hipError_t launch_jacobian(const ModelConst& P, int count, const double* x, const double* u, double* Jx,
                           double* Ju, hipStream_t s);
hipError_t launch_predict(const ModelConst& P, int count, const double* x, const double* u, double h,
                          int steps, double* xo, hipStream_t s);
// Plant simulator (plant_kernels.hip): x13 (B x 13) advanced in place over
// steps * substeps RK4 substeps of hs from t0 under the held u4 (B x 4).
//   mcf    per-kite model constants, field-major [kModelConstDoubles][B], or
//          nullptr: every kite takes P (kernel argument)
//   wind8  B x 8 [W0 (3) | A (3) | f_hz | phase], read for wind_mode 1
//          (constant wind, A ignored) and 2 (gust); mode 0: no wind
//   status B words (nullable), KITE_PLANT_NAN per kite, written on every call
constexpr int kModelConstDoubles = (int)(sizeof(ModelConst) / sizeof(double));
static_assert(sizeof(ModelConst) == kModelConstDoubles * sizeof(double), "ModelConst holds doubles only");
hipError_t launch_plant(const ModelConst& P, const double* mcf, int B, int wind_mode, const double* wind8,
                        double* x13, const double* u4, double t0, double hs, int steps, int substeps,
                        int32_t* status, hipStream_t s);
// the same plant behind a per-kite command line (k_plant_delay): line is B x
// KITE_DELAY_NLINE; u_cmd (and then tau) and u_applied may be null
hipError_t launch_plant_delay(const ModelConst& P, const double* mcf, int B, int wind_mode, const double* wind8,
                              double* x13, const double* u_cmd, const double* tau, double* line, double* u_applied,
                              double t0, double hs, int steps, int substeps, int32_t* status, hipStream_t s);
hipError_t launch_rk4_sens_items(const ModelConst& P, int sens_fp32, int count, int M, double h, const double* x,
                                 const double* u, double* xo, double* A, double* Bm, double* X2, double* AB,
                                 double* DEF, hipStream_t s);
hipError_t launch_closest_point(const RtiConst& C, int count, const double* pos, const double* guess,
                                double* theta, hipStream_t s);
// Chebyshev collocation evaluator (colloc_kernels.hip): constants of one formulation
struct CollocConst {
    int nodes, use_R;
    double t_scale, mayer_scale;
    double Q[3], R[4], W, vref;
    double Sx[15], Su[4], iSx[15], iSu[4];
    double path_R, path_alt, pq[4];
    int path_K, pad_;
    double pF[3][KITE_PATH_NC];
};
// tab = CompDiff (nodes x nodes, row-major) followed by the node weights (nodes)
hipError_t launch_colloc(const ModelConst& P, const CollocConst& C, int count, const double* tab, const double* z,
                         double* G, double* J, double* jac, hipStream_t s);
// batched EKF propagate (+ update when z != nullptr), in place on x and Pc (ekf_kernels.hip)
// mct: per-kite model constants, the controller's table ([count][kModelTableStride],
// kite b filters with row b), or nullptr: every kite takes P (kernel argument)
hipError_t launch_ekf(const ModelConst& P, const double* mct, int count, double dt, double* x, const double* u,
                      double* Pc, const double* z, const double* W, const double* V, hipStream_t s);
// Wind-estimating EKF (windekf_kernels.hip): `substeps` propagations of
// dt / substeps (+ one update when z != nullptr), in place on x16 (count x 16,
// [x13 | W3]) and Pc (count x 16 x 16); status: count words (nullable),
// KITE_EKF_* per kite, written on every call; mct as launch_ekf's
hipError_t launch_ekf_wind(const ModelConst& P, const double* mct, int count, double dt, int substeps, double* x16,
                           const double* u, double* Pc, const double* z, const double* W, const double* V,
                           int32_t* status, hipStream_t s);
// J (count x 13 x 16) = [df/dx | df/dW] under the winds w (count x 3)
hipError_t launch_jacobian_wind(const ModelConst& P, int count, const double* x, const double* u, const double* w,
                                double* J, hipStream_t s);
// dst (B x 3) <- B winds `stride` doubles apart at src, clamped to +-wmax, non-finite -> 0
hipError_t launch_wind_copy(int B, const double* src, int stride, double wmax, double* dst, hipStream_t s);
// Kinematic (pose-only) EKF (kinekf_kernels.hip, model: kin_model.hpp):
// `substeps` propagations of dt / substeps (+ one update when z != nullptr),
// in place on x13 and Pc (count x 13 x 13); frame: the motion-capture -> world
// change applied to a copy of z (host pointer, passed by value into the
// launch), or nullptr: z is a world pose; status as launch_ekf_wind's
struct PoseFrame;
hipError_t launch_ekf_kin(int count, double dt, int substeps, double* x13, double* Pc, const double* z,
                          const double* W, const double* V, const PoseFrame* frame, int32_t* status, hipStream_t s);
// x13 (count x 13) from two world poses dt apart (KiteEKF_Node::initialize);
// status: count words (nullable), KITE_EKF_INIT_BAD per kite, written on every call
hipError_t launch_ekf_kin_init(int count, double dt, const double* prev7, const double* next7, const PoseFrame* frame,
                               double* x13, int32_t* status, hipStream_t s);
// J (count x 13 x 13) = df/dx of the kinematic model
hipError_t launch_jacobian_kin(int count, const double* x, double* J, hipStream_t s);

}  // namespace kite
