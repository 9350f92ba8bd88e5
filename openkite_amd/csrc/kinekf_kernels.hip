// kinekf_kernels.hip -- the kinematic (pose-only) extended Kalman filter on gfx950.
//
// The filter the reference's estimator node flies: KiteEKF(Function, Function)
// (kiteEKF.cpp:54-72) over RigidBodyKinematics (kin_model.hpp).  It carries no
// aerodynamic constant: v_b and w_b are random walks, r and q follow the
// rigid-body kinematics, the 7 pose components are measured.
//
//   x13 = [v_b w_b r q],  P 13 x 13,  H = [0_{7x6} I_7]
//
//   [with a frame]  z <- frame(z)                  (optitrack2world, in registers)
//   [with z]        z_q <- -z_q if z_q . q_est < 0 (q and -q are one attitude)
//   per substep s of h = dt / substeps
//     A = I_13 + J(x) h,  x <- one RK4 step over h,  P <- A P A' + W
//   then, with a measurement z, one update (ekf_update.hpp, shared with
//   k_ekf and k_ekf_wind) and its containment tail (ekf_commit, there):
//     S = P[6:13, 6:13] + V (7 x 7 Cholesky in registers),
//     x <- x + P[:, 6:13] S^-1 (z - x[6:13]),  P <- P - P[:, 6:13] S^-1 P[6:13, :]
//     P <- (P + P') / 2
//
// Three deviations from the reference, all documented in DESIGN 4.13:
//   * the integrator is one RK4 step per substep over the dt the call is given;
//     the reference's CVODES integrates over a fixed 0.02 s whatever the
//     filter's dt is (kite.cpp:656-659 against kiteEKF.cpp:83-93);
//   * the measured quaternion is sign-aligned to the estimate (above);
//   * P is symmetrised after the update (ekf_commit, ekf_update.hpp, has the reason).
//
// Lane layout: the neighbours' -- 16 lanes per kite, 4 kites per wavefront,
// 64-thread blocks; lane j < 13 owns column j of P, lanes 13..15 carry zeros.
// A = I + J h is never formed as a matrix.  J has 49 non-zeros in rows 6..12
// (columns 0..2 and 9..12 of the r rows, 3..5 and 9..12 of the q rows), every
// lane holds x and so all of them in registers:
//   N = P A'   lane j needs row j of A: at most 7 entries off the unit
//              diagonal, selected into registers; the columns of P they
//              multiply come from LDS (7 reads per row instead of 13)
//   P+ = A N   column j of N is the lane's own: registers only, rows 0..5 of A
//              are the identity (no work), rows 6..12 cost 7 fma each
// so a substep is 13 x 7 + 7 x 7 = 140 fma per lane instead of 2 x 169, and one
// matrix (P) goes through LDS instead of two.  All sums run in index order on
// one lane: no atomics, no cross-lane reduction.
// LDS: row stride 16, kite stride 13 x 16 = 208 doubles (6656 bytes a block).
// A store (ds_write_b64: groups of 16 lanes, 32 banks of 4 bytes) puts a kite's
// 16 consecutive doubles on 32 different banks; a load (ds_read_b64: groups of
// 32 lanes, 64 banks) meets two kites 208 = 6 x 32 + 16 doubles apart, whose
// columns 0..12 fall on banks 0..25 and 32..57: no conflicts.
//
// Containment: the four kites of a block share every barrier.
// No lane returns early and no loop is left early; a frozen or out-of-range
// kite is predicated.  A kite whose estimate or covariance is non-finite on
// entry, or turns non-finite in a substep, keeps its last finite x and P
// (KITE_EKF_NAN); a kite whose innovation covariance has a pivot <= 0 or
// non-finite, or whose measurement is non-finite, keeps the propagated
// estimate (KITE_EKF_S_NOT_PD).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ekf_update.hpp"
#include "kin_model.hpp"
#include "kite_nmpc/kite_nmpc.h"
#include "rti_kernels.hpp"

namespace kite {

constexpr int KEKF_T = 64;             // threads per block = 4 kites x 16 lanes
constexpr int KEKF_N = 13;             // filter states
constexpr int KEKF_LD = 16;            // LDS row stride of the 13 x 13 matrix
constexpr int KEKF_KS = 13 * 16;       // LDS kite stride

__global__ __launch_bounds__(KEKF_T) void k_ekf_kin(int count, double dt, int substeps, double* __restrict__ x,
                                                    double* __restrict__ Pc, const double* __restrict__ z,
                                                    const double* __restrict__ W, const double* __restrict__ V,
                                                    PoseFrame frame, int use_frame, int32_t* __restrict__ status) {
    const int kk = threadIdx.x >> 4, j = threadIdx.x & 15;
    const int b = blockIdx.x * 4 + kk;
    const bool kite = b < count;
    const bool col = j < KEKF_N;             // the lane owns a column of P
    const int jc = col ? j : 0;              // a column index that is in range
    __shared__ double sP[4 * KEKF_KS];
    double* sp = sP + kk * KEKF_KS;
    const double h = dt / (double)substeps;

    // xv: every lane of the kite holds all of x; pcol: column j of P
    double xv[KEKF_N], pcol[KEKF_N], wcol[KEKF_N];
    for (int i = 0; i < KEKF_N; ++i) xv[i] = kite ? x[(size_t)b * KEKF_N + i] : 0.0;
    for (int i = 0; i < KEKF_N; ++i) pcol[i] = (kite && col) ? Pc[((size_t)b * KEKF_N + i) * KEKF_N + jc] : 0.0;
    for (int i = 0; i < KEKF_N; ++i) wcol[i] = col ? W[i * KEKF_N + jc] : 0.0;

    bool fin = true;
    for (int i = 0; i < KEKF_N; ++i) fin = fin && isfinite(xv[i]) && isfinite(pcol[i]);
    bool alive = !kite_any(!fin, kk);     // uniform over the kite's lanes
    const bool entry_ok = alive;
    int32_t flag = alive ? 0 : KITE_EKF_NAN;

    // the measurement: a copy in registers, moved to the world frame and
    // sign-aligned to the estimate on entry; the caller's z is only read
    double zv[7];
    bool zfin = true;
    if (z) {                                 // uniform over the grid
        for (int a = 0; a < 7; ++a) zv[a] = kite ? z[(size_t)b * 7 + a] : 0.0;
        if (use_frame) kin_frame(frame, zv);
        const double d = zv[3] * xv[9] + zv[4] * xv[10] + zv[5] * xv[11] + zv[6] * xv[12];
        if (d < 0.0)
            for (int a = 3; a < 7; ++a) zv[a] = -zv[a];
        for (int a = 0; a < 7; ++a) zfin = zfin && isfinite(zv[a]);
    }

    // row j of A off the diagonal: columns c0..c0+2 and 9..12
    const int c0 = (j >= 9 && j < KEKF_N) ? 3 : 0;

#pragma unroll 1
    for (int s = 0; s < substeps; ++s) {
        KinJac J;
        kin_jac(xv, J);
        // x+ = one RK4 step over h (every lane of the kite)
        double xn[KEKF_N];
        {
            double k[KEKF_N], xs[KEKF_N];
            for (int i = 0; i < KEKF_N; ++i) { xn[i] = xv[i]; xs[i] = xv[i]; }
#pragma unroll 1
            for (int st = 0; st < 4; ++st) {
                kin_rhs(xs, k);
                const double wa = (st == 0 || st == 3) ? h / 6.0 : h / 3.0;
                const double wn = (st < 2) ? 0.5 * h : h;
                for (int i = 6; i < KEKF_N; ++i) { xn[i] += wa * k[i]; xs[i] = xv[i] + wn * k[i]; }
            }
        }
        // the lane's row of A - I: ar[0..2] at columns c0.., ar[3..6] at columns 9..
        double ar[7];
        for (int m = 0; m < 7; ++m) ar[m] = 0.0;
        for (int a = 0; a < 3; ++a) {
            if (j == 6 + a) {
                for (int m = 0; m < 3; ++m) ar[m] = J.rv[a][m] * h;
                for (int m = 0; m < 4; ++m) ar[3 + m] = J.rq[a][m] * h;
            }
        }
        for (int a = 0; a < 4; ++a) {
            if (j == 9 + a) {
                for (int m = 0; m < 3; ++m) ar[m] = J.qw[a][m] * h;
                for (int m = 0; m < 4; ++m) ar[3 + m] = J.qq[a][m] * h;
            }
        }
        for (int i = 0; i < KEKF_N; ++i) sp[i * KEKF_LD + j] = pcol[i];
        __syncthreads();
        // N[:, j] = P[:, j] + sum_k P[:, k] (A - I)[j][k]
        double nn[KEKF_N];
        for (int i = 0; i < KEKF_N; ++i) {
            double t = 0.0;
            for (int m = 0; m < 3; ++m) t = fma(sp[i * KEKF_LD + c0 + m], ar[m], t);
            for (int m = 0; m < 4; ++m) t = fma(sp[i * KEKF_LD + 9 + m], ar[3 + m], t);
            nn[i] = pcol[i] + t;
        }
        // P+[:, j] = N[:, j] + (A - I) N[:, j] + Wcov[:, j]; rows 0..5 of A - I are zero
        double pn[KEKF_N];
        for (int i = 0; i < 6; ++i) pn[i] = nn[i] + wcol[i];
        for (int a = 0; a < 3; ++a) {
            double t = 0.0;
            for (int m = 0; m < 3; ++m) t = fma(J.rv[a][m] * h, nn[m], t);
            for (int m = 0; m < 4; ++m) t = fma(J.rq[a][m] * h, nn[9 + m], t);
            pn[6 + a] = (nn[6 + a] + t) + wcol[6 + a];
        }
        for (int a = 0; a < 4; ++a) {
            double t = 0.0;
            for (int m = 0; m < 3; ++m) t = fma(J.qw[a][m] * h, nn[3 + m], t);
            for (int m = 0; m < 4; ++m) t = fma(J.qq[a][m] * h, nn[9 + m], t);
            pn[9 + a] = (nn[9 + a] + t) + wcol[9 + a];
        }
        bool ok = true;
        for (int i = 6; i < KEKF_N; ++i) ok = ok && isfinite(xn[i]);
        for (int i = 0; i < KEKF_N; ++i) ok = ok && isfinite(pn[i]);
        const bool bad = kite_any(!ok, kk);
        if (alive && bad) { alive = false; flag = KITE_EKF_NAN; }   // keeps the last finite x, P
        if (alive) {
            for (int i = 6; i < KEKF_N; ++i) xv[i] = xn[i];
            for (int i = 0; i < KEKF_N; ++i) pcol[i] = pn[i];
        }
        __syncthreads();                     // sp is rewritten by the next substep
    }

    if (z) {                                 // uniform over the grid
        for (int i = 0; i < KEKF_N; ++i) sp[i * KEKF_LD + j] = pcol[i];
        __syncthreads();
        // the pose update and its containment tail: ekf_update.hpp
        double L[7][7];
        const bool pd = ekf_chol7<KEKF_LD>(sp, V, kite, L) && zfin;   // a non-finite measurement is a bad update
        double pu[KEKF_N], xu[KEKF_N], y[7];
        ekf_cov_update<KEKF_N, KEKF_LD>(sp, L, pcol, pu);
        for (int a = 0; a < 7; ++a) y[a] = zv[a] - xv[6 + a];
        ekf_state_update<KEKF_N, KEKF_LD>(sp, L, xv, y, xu);
        ekf_commit<KEKF_N, KEKF_LD>(sp, j, jc, kk, alive, pd, pu, xu, pcol, xv, flag);
    }
    // a kite that was non-finite on entry is left untouched; one frozen in a
    // substep stores the last finite x and P it holds
    if (kite && col && entry_ok)
        for (int i = 0; i < KEKF_N; ++i) Pc[((size_t)b * KEKF_N + i) * KEKF_N + jc] = pcol[i];
    if (kite && entry_ok && j == 0)
        for (int i = 0; i < KEKF_N; ++i) x[(size_t)b * KEKF_N + i] = xv[i];
    if (kite && j == 0 && status) status[b] = flag;
}

hipError_t launch_ekf_kin(int count, double dt, int substeps, double* x13, double* Pc, const double* z,
                          const double* W, const double* V, const PoseFrame* frame, int32_t* status, hipStream_t s) {
    PoseFrame F = {};
    if (frame) F = *frame;
    hipLaunchKernelGGL(k_ekf_kin, dim3((count + 3) / 4), dim3(KEKF_T), 0, s, count, dt, substeps, x13, Pc, z, W, V, F,
                       frame ? 1 : 0, status);
    return hipGetLastError();
}

// The two-pose initialisation (KiteEKF_Node::initialize, ekf_node.cpp:68-132):
// one lane per kite.  q_new is sign-aligned to q_prev for dq only; the state
// keeps the pose as measured.
__global__ __launch_bounds__(64) void k_ekf_kin_init(int count, double dt, const double* __restrict__ prev,
                                                     const double* __restrict__ next, PoseFrame frame, int use_frame,
                                                     double* __restrict__ x, int32_t* __restrict__ status) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= count) return;                  // no barrier in this kernel
    double mp[7], mn[7];
    for (int a = 0; a < 7; ++a) { mp[a] = prev[(size_t)b * 7 + a]; mn[a] = next[(size_t)b * 7 + a]; }
    if (use_frame) { kin_frame(frame, mp); kin_frame(frame, mn); }
    bool ok = isfinite(dt) && dt > 0.0;
    for (int a = 0; a < 7; ++a) ok = ok && isfinite(mp[a]) && isfinite(mn[a]);
    // v_b = vec( conj(q_prev) (x) [0, rdot] (x) q_prev )
    double rd[3], vb[3];
    for (int i = 0; i < 3; ++i) rd[i] = (mn[i] - mp[i]) / dt;
    const double qc[4] = {mp[3], -mp[4], -mp[5], -mp[6]};
    kin_rot(qc, rd, vb);
    // w_b = (2 / dt) vec( conj(q_prev) (x) q_new - [1, 0, 0, 0] )
    const double d = mp[3] * mn[3] + mp[4] * mn[4] + mp[5] * mn[5] + mp[6] * mn[6];
    const double sg = d < 0.0 ? -1.0 : 1.0;
    const double qn[4] = {sg * mn[3], sg * mn[4], sg * mn[5], sg * mn[6]};
    double dq[4];
    kin_qmul(qc, qn, dq);
    const double c = 2.0 / dt;
    if (ok) {
        double* xo = x + (size_t)b * KEKF_N;
        for (int i = 0; i < 3; ++i) { xo[i] = vb[i]; xo[3 + i] = c * dq[1 + i]; }
        for (int a = 0; a < 7; ++a) xo[6 + a] = mn[a];
    }
    if (status) status[b] = ok ? 0 : KITE_EKF_INIT_BAD;
}

hipError_t launch_ekf_kin_init(int count, double dt, const double* prev7, const double* next7, const PoseFrame* frame,
                               double* x13, int32_t* status, hipStream_t s) {
    PoseFrame F = {};
    if (frame) F = *frame;
    hipLaunchKernelGGL(k_ekf_kin_init, dim3((count + 63) / 64), dim3(64), 0, s, count, dt, prev7, next7, F,
                       frame ? 1 : 0, x13, status);
    return hipGetLastError();
}

// J (count x 13 x 13, row-major) = df/dx of the kinematic model: the filter's
// Jacobian pass, one lane per (kite, row)
__global__ __launch_bounds__(64) void k_jacobian_kin(int count, const double* __restrict__ x, double* __restrict__ Jo) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int b = t >> 4, i = t & 15;
    if (b >= count || i >= KEKF_N) return;   // no barrier in this kernel
    double xv[KEKF_N];
    for (int k = 0; k < KEKF_N; ++k) xv[k] = x[(size_t)b * KEKF_N + k];
    KinJac J;
    kin_jac(xv, J);
    double row[KEKF_N];
    for (int k = 0; k < KEKF_N; ++k) row[k] = 0.0;
    for (int a = 0; a < 3; ++a)
        if (i == 6 + a) {
            for (int m = 0; m < 3; ++m) row[m] = J.rv[a][m];
            for (int m = 0; m < 4; ++m) row[9 + m] = J.rq[a][m];
        }
    for (int a = 0; a < 4; ++a)
        if (i == 9 + a) {
            for (int m = 0; m < 3; ++m) row[3 + m] = J.qw[a][m];
            for (int m = 0; m < 4; ++m) row[9 + m] = J.qq[a][m];
        }
    for (int k = 0; k < KEKF_N; ++k) Jo[((size_t)b * KEKF_N + i) * KEKF_N + k] = row[k];
}

hipError_t launch_jacobian_kin(int count, const double* x, double* J, hipStream_t s) {
    hipLaunchKernelGGL(k_jacobian_kin, dim3((count + 3) / 4), dim3(64), 0, s, count, x, J);
    return hipGetLastError();
}

}  // namespace kite
