// ekf_kernels.hip -- batched extended Kalman filter of the kite
// on gfx950: KiteEKF::propagate + KiteEKF::_estimate
// (src/kite_estimation/kiteEKF.cpp:75-126) for `count` kites in one launch.
//
//   propagate  x+ = RK4(x, u, dt) (one step, kite.cpp:332-338),
//              A  = I + J(x) dt,  P+ = A P A' + W
//   update     y = z - H x+,  S = H P+ H' + V,  K = P+ H' S^-1,
//              x = x+ + K y,  P = (I - K H) P+      with H = [0_{7x6} I_7]
//
// Lane layout: one lane per (kite, column j of the 13 x 13 matrices); 16 lanes
// per kite (13 used), 4 kites per wavefront.  Lane j computes column j of the
// Jacobian with one dual-number pass of the RHS, then column j of A P and of
// A P A' from the matrices shared through LDS (13 x 14 per kite, LDS
// broadcast reads); the 7 x 7 innovation covariance is factored per lane in
// registers.  HBM per kite: x, u, z, P in and x, P out = 2 x 1.4 KB.
// The update (Cholesky, solves, the two gain products) is ekf_update.hpp's,
// shared with k_ekf_wind and k_ekf_kin; this filter does not check the pivots
// and does not symmetrise P.
#include <hip/hip_runtime.h>
#include <math.h>

#include "ekf_update.hpp"
#include "kite_model.hpp"
#include "rti_kernels.hpp"

namespace kite {

constexpr int EKF_T = 64;           // threads per block = 4 kites x 16 lanes
constexpr int EKF_PK_T = 16;        // k_ekf_pk: one kite per block
constexpr int EKF_LD = 14;          // LDS row stride of a 13 x 13 matrix

__global__ __launch_bounds__(EKF_T, 2) void k_ekf(ModelConst P, int count, double dt, double* __restrict__ x,
                                                   const double* __restrict__ u, double* __restrict__ Pc,
                                                   const double* __restrict__ z, const double* __restrict__ W,
                                                   const double* __restrict__ V) {
    const int kk = threadIdx.x >> 4, j = threadIdx.x & 15;
    const int b = blockIdx.x * 4 + kk;
    const bool kite = b < count;
#include "ekf_body.inc"
}

// k_ekf with a model per kite: kite b filters with row b of the controller's
// table mct ([count][kModelTableStride], rti_kernels.hpp).  A block is ONE
// kite: 16 threads, the kite's 16 lanes, grid `count`; the row is wave-uniform
// and arrives by scalar loads (model_row, as in k_prologue_pk) into the SGPRs
// that hold k_ekf's kernel argument, so the kernel has k_ekf's registers and
// instructions and its estimates bit for bit.  (With k_ekf's four kites per
// wave the 47 constants are lane-varying.  In VGPRs they cost 73 registers and
// the second wave per SIMD without scratch, but the compiler then pairs other
// multiplies and adds into fused ones: same instruction counts, results one
// ulp off k_ekf's.  DESIGN 4.11.)  kk is 0 and no kite is out of range; the
// included body keeps its predication.
__global__ __launch_bounds__(EKF_T, 2) void k_ekf_pk(const double* __restrict__ mct, int count, double dt,
                                                      double* __restrict__ x, const double* __restrict__ u,
                                                      double* __restrict__ Pc, const double* __restrict__ z,
                                                      const double* __restrict__ W, const double* __restrict__ V) {
    const int kk = threadIdx.x >> 4, j = threadIdx.x & 15;      // kk = 0: 16 threads
    const int b = blockIdx.x + kk;
    const bool kite = b < count;
    const ModelConst P = model_row(mct, blockIdx.x);
#include "ekf_body.inc"
}

hipError_t launch_ekf(const ModelConst& P, const double* mct, int count, double dt, double* x, const double* u,
                      double* Pc, const double* z, const double* W, const double* V, hipStream_t s) {
    if (mct)
        hipLaunchKernelGGL(k_ekf_pk, dim3(count), dim3(EKF_PK_T), 0, s, mct, count, dt, x, u, Pc, z, W, V);
    else
        hipLaunchKernelGGL(k_ekf, dim3((count + 3) / 4), dim3(EKF_T), 0, s, P, count, dt, x, u, Pc, z, W, V);
    return hipGetLastError();
}

}  // namespace kite
