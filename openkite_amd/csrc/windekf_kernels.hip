// windekf_kernels.hip -- the wind-estimating extended Kalman filter on gfx950.
//
// k_ekf (ekf_kernels.hip) estimates the 13 kite states with the wind-free
// reference model.  k_ekf_wind carries a constant world-frame wind W (m/s) as
// three more filter states, a random walk (W_dot = 0):
//
//   x16 = [x13 | W3],  P 16 x 16,  H = [0_{7x6} I_7 0_{7x3}]  (r and q measured)
//
//   per substep s of h = dt / substeps
//     A   = I_16 + J h,  J = [df/dx | df/dW ; 0_{3x16}] under the estimated wind
//     x13 <- one RK4 step of kite_rhs<double, true> under that wind, W unchanged
//     P   <- A P A' + Wcov
//   then, with a measurement z, one update as k_ekf does it:
//     S = P[6:13, 6:13] + V (7 x 7 Cholesky in registers),
//     x <- x + P[:, 6:13] S^-1 (z - x[6:13]),  P <- P - P[:, 6:13] S^-1 P[6:13, :]
//   and, beyond k_ekf, P <- (P + P') / 2 after the update (see there)
//
// Lane layout: k_ekf's -- lane j of a kite's 16 owns column j of the 16 x 16
// matrices, 4 kites per wavefront, 64-thread blocks -- with every lane busy:
// lane j seeds the tangent of x_j (j < 13) or of W_{j-13} in one dual-number
// pass of kite_rhs<Dual, true, Dual>.  A and A P are shared through LDS (row
// stride 17, kite stride 276 doubles: the four kites' broadcast reads fall on
// different banks).  The time loop over the substeps runs in the kernel, so a
// control period is one launch.
//
// Containment: the four kites of a block share every barrier.  No lane
// returns early and no loop is left early; a frozen or out-of-range kite is
// predicated and walks the same barriers.  A kite whose estimate or covariance
// is non-finite on entry, or turns non-finite in a substep, keeps its last
// finite x16 and P (KITE_EKF_NAN); a kite whose innovation covariance has a
// pivot <= 0 or non-finite keeps the propagated estimate (KITE_EKF_S_NOT_PD).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kite_model.hpp"
#include "kite_nmpc/kite_nmpc.h"
#include "rti_kernels.hpp"

namespace kite {

constexpr int WEKF_T = 64;            // threads per block = 4 kites x 16 lanes
constexpr int WEKF_N = 16;            // filter states
constexpr int WEKF_LD = 17;           // LDS row stride of a 16 x 16 matrix
constexpr int WEKF_KS = 16 * 17 + 4;  // LDS kite stride

// column j (0..15) of [df/dx | df/dW] at (x, u, wind w): one dual-number pass
__device__ __forceinline__ void wind_jac_col(const ModelConst& P, const double* xv, const double* uv,
                                             const double* wv, int j, double* col) {
    Dual xx[NK], uu[NKU], ww[3], ff[NK];
    for (int i = 0; i < NK; ++i) xx[i] = mk(xv[i], i == j ? 1.0 : 0.0);
    for (int i = 0; i < NKU; ++i) uu[i] = mk(uv[i], 0.0);
    for (int i = 0; i < 3; ++i) ww[i] = mk(wv[i], NK + i == j ? 1.0 : 0.0);
    kite_rhs<Dual, true, Dual>(P, xx, uu, ff, ww);
    for (int i = 0; i < NK; ++i) col[i] = ff[i].t;
}

// true when any of the calling kite's 16 lanes passes bad (kk: kite of the wave)
__device__ __forceinline__ bool kite_any(bool bad, int kk) {
    const unsigned long long m = __ballot(bad);
    return ((m >> (kk * 16)) & 0xFFFFull) != 0;
}

__global__ __launch_bounds__(WEKF_T) void k_ekf_wind(ModelConst P, int count, double dt, int substeps,
                                                     double* __restrict__ x, const double* __restrict__ u,
                                                     double* __restrict__ Pc, const double* __restrict__ z,
                                                     const double* __restrict__ W, const double* __restrict__ V,
                                                     int32_t* __restrict__ status) {
    __shared__ double sA[4 * WEKF_KS];
    __shared__ double sN[4 * WEKF_KS];
    const int kk = threadIdx.x >> 4, j = threadIdx.x & 15;
    const int b = blockIdx.x * 4 + kk;
    const bool kite = b < count;
    double* sa = sA + kk * WEKF_KS;
    double* sn = sN + kk * WEKF_KS;
    const double h = dt / (double)substeps;

    // xv: [x13 | W3], every lane of the kite holds all of it; pcol: column j of P
    double xv[WEKF_N], uv[NKU], pcol[WEKF_N], wcol[WEKF_N];
    for (int i = 0; i < WEKF_N; ++i) xv[i] = kite ? x[(size_t)b * WEKF_N + i] : 0.0;
    for (int i = 0; i < NKU; ++i) uv[i] = kite ? u[(size_t)b * NKU + i] : 0.0;
    for (int i = 0; i < WEKF_N; ++i) pcol[i] = kite ? Pc[((size_t)b * WEKF_N + i) * WEKF_N + j] : 0.0;
    for (int i = 0; i < WEKF_N; ++i) wcol[i] = W[i * WEKF_N + j];

    bool fin = true;
    for (int i = 0; i < WEKF_N; ++i) fin = fin && isfinite(xv[i]) && isfinite(pcol[i]);
    bool alive = !kite_any(!fin, kk);         // uniform over the kite's lanes
    const bool entry_ok = alive;
    int32_t flag = alive ? 0 : KITE_EKF_NAN;

#pragma unroll 1
    for (int s = 0; s < substeps; ++s) {
        // column j of A = I + J h at the estimate; rows 13..15: W_dot = 0
        {
            double jc[NK];
            wind_jac_col(P, xv, uv, xv + NK, j, jc);
            for (int i = 0; i < NK; ++i) sa[i * WEKF_LD + j] = jc[i] * h + (i == j ? 1.0 : 0.0);
            for (int i = NK; i < WEKF_N; ++i) sa[i * WEKF_LD + j] = (i == j ? 1.0 : 0.0);
        }
        // x13+ = one RK4 step over h under the estimated wind (every lane of the kite)
        double xn[NK];
        {
            double k[NK], xs[NK];
            for (int i = 0; i < NK; ++i) { xn[i] = xv[i]; xs[i] = xv[i]; }
#pragma unroll 1
            for (int st = 0; st < 4; ++st) {
                kite_rhs<double, true>(P, xs, uv, k, xv + NK);
                const double wa = (st == 0 || st == 3) ? h / 6.0 : h / 3.0;
                const double wn = (st < 2) ? 0.5 * h : h;
                for (int i = 0; i < NK; ++i) { xn[i] += wa * k[i]; xs[i] = xv[i] + wn * k[i]; }
            }
        }
        __syncthreads();
        // (A P)[:, j]
        for (int i = 0; i < WEKF_N; ++i) {
            double t = 0.0;
            for (int k = 0; k < WEKF_N; ++k) t = fma(sa[i * WEKF_LD + k], pcol[k], t);
            sn[i * WEKF_LD + j] = t;
        }
        __syncthreads();
        // P+[:, j] = sum_k (A P)[:, k] A[j][k] + Wcov[:, j]
        double pn[WEKF_N];
        for (int i = 0; i < WEKF_N; ++i) {
            double t = wcol[i];
            for (int k = 0; k < WEKF_N; ++k) t = fma(sn[i * WEKF_LD + k], sa[j * WEKF_LD + k], t);
            pn[i] = t;
        }
        bool ok = true;
        for (int i = 0; i < NK; ++i) ok = ok && isfinite(xn[i]);
        for (int i = 0; i < WEKF_N; ++i) ok = ok && isfinite(pn[i]);
        const bool bad = kite_any(!ok, kk);
        if (alive && bad) { alive = false; flag = KITE_EKF_NAN; }   // keeps the last finite x16, P
        if (alive) {
            for (int i = 0; i < NK; ++i) xv[i] = xn[i];
            for (int i = 0; i < WEKF_N; ++i) pcol[i] = pn[i];
        }
        __syncthreads();                     // sa, sn are rewritten by the next substep
    }

    if (z) {                                 // uniform over the grid
        for (int i = 0; i < WEKF_N; ++i) sn[i * WEKF_LD + j] = pcol[i];
        __syncthreads();
        // S = P+[6:13, 6:13] + V, Cholesky in registers (lower), every lane its own copy
        double L[7][7];
        for (int a = 0; a < 7; ++a)
            for (int c = 0; c <= a; ++c) L[a][c] = kite ? sn[(6 + a) * WEKF_LD + 6 + c] + V[a * 7 + c] : (a == c);
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
        auto solve = [&](double r[7]) {          // r <- S^-1 r
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
        };
        // P[:, j] = P+[:, j] - P+[:, 6:13] S^-1 P+[6:13, j]
        double pu[WEKF_N], xu[WEKF_N];
        {
            double c7[7];
            for (int a = 0; a < 7; ++a) c7[a] = pcol[6 + a];
            solve(c7);
            for (int i = 0; i < WEKF_N; ++i) {
                double t = pcol[i];
                for (int a = 0; a < 7; ++a) t = fma(-sn[i * WEKF_LD + 6 + a], c7[a], t);
                pu[i] = t;
            }
        }
        // x = x+ + P+[:, 6:13] S^-1 (z - x+[6:13])
        {
            double y[7];
            for (int a = 0; a < 7; ++a) y[a] = (kite ? z[(size_t)b * 7 + a] : 0.0) - xv[6 + a];
            solve(y);
            for (int i = 0; i < WEKF_N; ++i) {
                double t = xv[i];
                for (int a = 0; a < 7; ++a) t = fma(sn[i * WEKF_LD + 6 + a], y[a], t);
                xu[i] = t;
            }
        }
        bool ok = true;
        for (int i = 0; i < WEKF_N; ++i) ok = ok && isfinite(pu[i]) && isfinite(xu[i]);
        const bool bad = kite_any(!ok, kk);
        if (alive && !pd) flag |= KITE_EKF_S_NOT_PD;            // update skipped
        else if (alive && bad) flag |= KITE_EKF_NAN;            // keeps the propagated estimate
        const bool updated = alive && pd && !bad;
        if (updated) {
            for (int i = 0; i < WEKF_N; ++i) { pcol[i] = pu[i]; xv[i] = xu[i]; }
        }
        // P <- (P + P') / 2 of an updated kite.  S is factored from its lower
        // triangle alone, so the update does not damp an antisymmetric part of
        // P: rounding seeds one and every further update multiplies it (by 1.4
        // to 1.6 per period in the open-loop run of the tests: 1e-15 becomes
        // 1e-10 within 40 periods and O(1) within 100).  Both halves of a pair
        // add the same two numbers, so P leaves exactly symmetric.
        __syncthreads();                     // every lane is done with P+ in sn
        for (int i = 0; i < WEKF_N; ++i) sn[i * WEKF_LD + j] = pcol[i];
        __syncthreads();
        if (updated)
            for (int i = 0; i < WEKF_N; ++i) pcol[i] = 0.5 * (pcol[i] + sn[j * WEKF_LD + i]);
    }
    // a kite that was non-finite on entry is left untouched; one frozen in a
    // substep stores the last finite x16 and P it holds
    if (kite && entry_ok)
        for (int i = 0; i < WEKF_N; ++i) Pc[((size_t)b * WEKF_N + i) * WEKF_N + j] = pcol[i];
    if (kite && entry_ok && j == 0)
        for (int i = 0; i < WEKF_N; ++i) x[(size_t)b * WEKF_N + i] = xv[i];
    if (kite && j == 0 && status) status[b] = flag;
}

hipError_t launch_ekf_wind(const ModelConst& P, int count, double dt, int substeps, double* x16, const double* u,
                           double* Pc, const double* z, const double* W, const double* V, int32_t* status,
                           hipStream_t s) {
    hipLaunchKernelGGL(k_ekf_wind, dim3((count + 3) / 4), dim3(WEKF_T), 0, s, P, count, dt, substeps, x16, u, Pc, z,
                       W, V, status);
    return hipGetLastError();
}

// J (count x 13 x 16, row-major) = [df/dx | df/dW] under wind w: the filter's
// Jacobian pass, one lane per (kite, column)
__global__ __launch_bounds__(64) void k_jacobian_wind(ModelConst P, int count, const double* __restrict__ x,
                                                      const double* __restrict__ u, const double* __restrict__ w,
                                                      double* __restrict__ J) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int b = t >> 4, j = t & 15;
    if (b >= count) return;
    double xv[NK], uv[NKU], wv[3], jc[NK];
    for (int i = 0; i < NK; ++i) xv[i] = x[(size_t)b * NK + i];
    for (int i = 0; i < NKU; ++i) uv[i] = u[(size_t)b * NKU + i];
    for (int i = 0; i < 3; ++i) wv[i] = w[(size_t)b * 3 + i];
    wind_jac_col(P, xv, uv, wv, j, jc);
    for (int i = 0; i < NK; ++i) J[((size_t)b * NK + i) * WEKF_N + j] = jc[i];
}

hipError_t launch_jacobian_wind(const ModelConst& P, int count, const double* x, const double* u, const double* w,
                                double* J, hipStream_t s) {
    hipLaunchKernelGGL(k_jacobian_wind, dim3((count + 3) / 4), dim3(64), 0, s, P, count, x, u, w, J);
    return hipGetLastError();
}

// dst (B x 3) <- the B winds that sit `stride` doubles apart at src, each
// component clamped to +-wmax, a non-finite one replaced by 0
__global__ __launch_bounds__(64) void k_wind_copy(int B, const double* __restrict__ src, int stride, double wmax,
                                                  double* __restrict__ dst) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= B * 3) return;
    const int b = t / 3, c = t - b * 3;
    double v = src[(size_t)b * stride + c];
    if (!isfinite(v)) v = 0.0;
    dst[t] = fmin(fmax(v, -wmax), wmax);
}

hipError_t launch_wind_copy(int B, const double* src, int stride, double wmax, double* dst, hipStream_t s) {
    hipLaunchKernelGGL(k_wind_copy, dim3((B * 3 + 63) / 64), dim3(64), 0, s, B, src, stride, wmax, dst);
    return hipGetLastError();
}

}  // namespace kite
