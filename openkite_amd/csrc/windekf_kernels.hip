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
//   then, with a measurement z, one update (ekf_update.hpp, shared with k_ekf
//   and k_ekf_kin):
//     S = P[6:13, 6:13] + V (7 x 7 Cholesky in registers),
//     x <- x + P[:, 6:13] S^-1 (z - x[6:13]),  P <- P - P[:, 6:13] S^-1 P[6:13, :]
//   and, beyond k_ekf, the containment tail: the flags and P <- (P + P') / 2
//   after the update (this filter's own copy of ekf_commit's statements;
//   the reason for the symmetrisation is written at ekf_commit)
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

#include "ekf_update.hpp"
#include "kite_model.hpp"
#include "kite_nmpc/kite_nmpc.h"
#include "rti_kernels.hpp"

namespace kite {

constexpr int WEKF_T = 64;            // threads per block = 4 kites x 16 lanes
constexpr int WEKF_PK_T = 16;         // k_ekf_wind_pk: one kite per block
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

__global__ __launch_bounds__(WEKF_T) void k_ekf_wind(ModelConst P, int count, double dt, int substeps,
                                                     double* __restrict__ x, const double* __restrict__ u,
                                                     double* __restrict__ Pc, const double* __restrict__ z,
                                                     const double* __restrict__ W, const double* __restrict__ V,
                                                     int32_t* __restrict__ status) {
    const int kk = threadIdx.x >> 4, j = threadIdx.x & 15;
    const int b = blockIdx.x * 4 + kk;
    const bool kite = b < count;
#include "windekf_body.inc"
}

// k_ekf_wind with a model per kite: kite b filters with row b of the
// controller's table mct ([count][kModelTableStride], rti_kernels.hpp).  With
// four kites per wave the 47 constants would be lane-varying: 94 more VGPRs in
// a kernel that sits at 458 of 512, which spills (30 VGPRs, 124 bytes of
// scratch), and lane-varying constants change which multiplies and adds the
// compiler fuses (k_ekf_pk, ekf_kernels.hip).  So here a block is ONE kite: 16 threads, the kite's 16 columns, grid
// `count`; the row is wave-uniform and arrives by scalar loads (model_row, as
// in k_prologue_pk), and the kernel has k_ekf_wind's registers and
// instructions.  kk is 0 and no kite is out of range; the included body keeps
// its predication and walks the same barriers.
__global__ __launch_bounds__(WEKF_T) void k_ekf_wind_pk(const double* __restrict__ mct, int count, double dt,
                                                        int substeps, double* __restrict__ x,
                                                        const double* __restrict__ u, double* __restrict__ Pc,
                                                        const double* __restrict__ z, const double* __restrict__ W,
                                                        const double* __restrict__ V, int32_t* __restrict__ status) {
    const int kk = threadIdx.x >> 4, j = threadIdx.x & 15;      // kk = 0: 16 threads
    const int b = blockIdx.x + kk;
    const bool kite = b < count;
    const ModelConst P = model_row(mct, blockIdx.x);
#include "windekf_body.inc"
}

hipError_t launch_ekf_wind(const ModelConst& P, const double* mct, int count, double dt, int substeps, double* x16,
                           const double* u, double* Pc, const double* z, const double* W, const double* V,
                           int32_t* status, hipStream_t s) {
    if (mct)
        hipLaunchKernelGGL(k_ekf_wind_pk, dim3(count), dim3(WEKF_PK_T), 0, s, mct, count, dt, substeps, x16, u,
                           Pc, z, W, V, status);
    else
        hipLaunchKernelGGL(k_ekf_wind, dim3((count + 3) / 4), dim3(WEKF_T), 0, s, P, count, dt, substeps, x16, u, Pc,
                           z, W, V, status);
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
