// ekf_update.hpp -- what the batched EKFs share on the device: the pose
// measurement update of k_ekf / k_ekf_pk (ekf_body.inc), k_ekf_wind /
// k_ekf_wind_pk (windekf_body.inc) and k_ekf_kin (kinekf_kernels.hip), the
// per-kite ballot, and the containment tail ekf_commit.  k_ekf_kin calls
// ekf_commit; the wind filter keeps the same statements as its own copy,
// because through the function k_ekf_wind_pk came out about 1.2 % slower
// (profiles/ekf_update_probe.json).  The RK4 step and the A P A' + W products
// stay with each kernel: inlined through a shared step function the model's
// right-hand side pairs other multiplies and adds into fused ones (in k_ekf
// a*a + b*b fuses the other product, k_ekf_wind has 1766 fused operations
// instead of 1763), and k_ekf's products are predicated and read W from
// memory where k_ekf_wind's are not.
//
//   H = [0_{7x6} I_7 0...]:  S = P[6:13, 6:13] + V,
//   x <- x + P[:, 6:13] S^-1 (z - x[6:13]),  P <- P - P[:, 6:13] S^-1 P[6:13, :]
//
// Lane layout of every caller: 16 lanes per kite, 4 kites per wavefront, lane j
// owns column j of P; the kite's P+ sits in LDS at sp with row stride LD and
// every lane factors its own copy of S in registers.  Nothing here owns LDS;
// only ekf_commit walks barriers.  All sums run in index order on one lane.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kite_nmpc/kite_nmpc.h"

namespace kite {

// true when any of the calling kite's 16 lanes passes bad (kk: kite of the wave)
__device__ __forceinline__ bool kite_any(bool bad, int kk) {
    const unsigned long long m = __ballot(bad);
    return ((m >> (kk * 16)) & 0xFFFFull) != 0;
}

// L <- chol(S), S = P+[6:13, 6:13] + V from the kite's matrix at sp (lower; the
// identity for an out-of-range kite).  Returns whether every pivot is > 0 and finite.
template <int LD>
__device__ __forceinline__ bool ekf_chol7(const double* sp, const double* V, bool kite, double (&L)[7][7]) {
    for (int a = 0; a < 7; ++a)
        for (int c = 0; c <= a; ++c) L[a][c] = kite ? sp[(6 + a) * LD + 6 + c] + V[a * 7 + c] : (a == c);
    bool pd = true;
    for (int c = 0; c < 7; ++c) {
        double d = L[c][c];
        for (int k = 0; k < c; ++k) d -= L[c][k] * L[c][k];
        pd = pd && (d > 0.0) && isfinite(d);
        d = sqrt(d);
        L[c][c] = d;
        for (int a = c + 1; a < 7; ++a) {
            double t = L[a][c];
            for (int k = 0; k < c; ++k) t -= L[a][k] * L[c][k];
            L[a][c] = t / d;
        }
    }
    return pd;
}

// r <- S^-1 r
__device__ __forceinline__ void ekf_solve7(const double (&L)[7][7], double (&r)[7]) {
    for (int a = 0; a < 7; ++a) {
        double t = r[a];
        for (int k = 0; k < a; ++k) t -= L[a][k] * r[k];
        r[a] = t / L[a][a];
    }
    for (int a = 6; a >= 0; --a) {
        double t = r[a];
        for (int k = a + 1; k < 7; ++k) t -= L[k][a] * r[k];
        r[a] = t / L[a][a];
    }
}

// pu = P+[:, j] - P+[:, 6:13] S^-1 P+[6:13, j]  (pcol: column j of P+; pu may be pcol)
template <int N, int LD>
__device__ __forceinline__ void ekf_cov_update(const double* sp, const double (&L)[7][7], const double* pcol,
                                               double* pu) {
    double c7[7];
    for (int a = 0; a < 7; ++a) c7[a] = pcol[6 + a];
    ekf_solve7(L, c7);
    for (int i = 0; i < N; ++i) {
        double t = pcol[i];
        for (int a = 0; a < 7; ++a) t = fma(-sp[i * LD + 6 + a], c7[a], t);
        pu[i] = t;
    }
}

// xu = x+ + P+[:, 6:13] S^-1 y, y = z - x+[6:13] (overwritten; xu may be xv)
template <int N, int LD>
__device__ __forceinline__ void ekf_state_update(const double* sp, const double (&L)[7][7], const double* xv,
                                                 double (&y)[7], double* xu) {
    ekf_solve7(L, y);
    for (int i = 0; i < N; ++i) {
        double t = xv[i];
        for (int a = 0; a < 7; ++a) t = fma(sp[i * LD + 6 + a], y[a], t);
        xu[i] = t;
    }
}

// The tail of an update with containment: the kite takes (pu, xu) into (pcol,
// xv) when it is alive, S was positive definite (pd) and every lane's pu, xu
// are finite; otherwise it keeps the propagated estimate and flag says why.
// Then P <- (P + P') / 2 of an updated kite, through sp (lane j stores column
// j, reads row jc: jc is j, or an in-range index for a lane without a column).
// S is factored from its lower triangle alone, so the update does not damp an
// antisymmetric part of P: rounding seeds one and every further update
// multiplies it (by 1.4 to 1.6 per period in the open-loop run of the wind
// filter's tests: 1e-15 becomes 1e-10 within 40 periods and O(1) within 100).
// Both halves of a pair add the same two numbers, so P leaves exactly symmetric.
// Every lane of the block walks the two barriers: call it unconditionally
// under a condition that is uniform over the grid.
template <int N, int LD>
__device__ __forceinline__ void ekf_commit(double* sp, int j, int jc, int kk, bool alive, bool pd, const double* pu,
                                           const double* xu, double* pcol, double* xv, int32_t& flag) {
    bool ok = true;
    for (int i = 0; i < N; ++i) ok = ok && isfinite(pu[i]) && isfinite(xu[i]);
    const bool bad = kite_any(!ok, kk);
    if (alive && !pd) flag |= KITE_EKF_S_NOT_PD;            // update skipped
    else if (alive && bad) flag |= KITE_EKF_NAN;            // keeps the propagated estimate
    const bool updated = alive && pd && !bad;
    if (updated) {
        for (int i = 0; i < N; ++i) { pcol[i] = pu[i]; xv[i] = xu[i]; }
    }
    __syncthreads();                     // every lane is done with P+ in sp
    for (int i = 0; i < N; ++i) sp[i * LD + j] = pcol[i];
    __syncthreads();
    if (updated)
        for (int i = 0; i < N; ++i) pcol[i] = 0.5 * (pcol[i] + sp[jc * LD + i]);
}

}  // namespace kite
