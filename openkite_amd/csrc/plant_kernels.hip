// plant_kernels.hip -- the batched plant simulator for gfx950.
//
// The openKITE simulator node (src/kite_model/simulator.cpp) integrates the
// kite ODE at 50 Hz under the control it received last.  k_plant does that for
// a whole batch on the device: one lane per kite, one launch per control
// period (the time loop over steps x substeps RK4 substeps runs in the
// kernel), with what makes the plant differ from the controller's model:
//   * model constants per kite (a ModelConst per kite, stored field-major
//     [field][kite] so that a wavefront's loads coalesce; loaded once into the
//     lane's registers),
//   * a world-frame wind per kite with a sinusoidal gust,
//     W(t) = W0 + A sin(2 pi f t + phase), evaluated at every RK4 stage time,
//   * containment: a kite whose state turns non-finite keeps its last finite
//     state and is flagged (KITE_PLANT_NAN); the other lanes are not affected.
// The integrator repeats rk4_primal (rti_kernels.hip) operation for operation
// on the 13 kite states: the nominal plant (controller's constants, no wind)
// is k_predict's arithmetic.  theta / thetadot are the controller's states,
// not the plant's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kite_model.hpp"
#include "kite_nmpc/kite_nmpc.h"
#include "rti_kernels.hpp"

namespace kite {

enum : int { PLANT_CALM = 0, PLANT_WIND = 1, PLANT_GUST = 2 };

// start time of substep k: the product rounded, then the sum (no fused
// multiply-add), so that a call at t0' = t0 + k0 hs as the host computes it
// continues an earlier call
__device__ __forceinline__ double plant_time(double t0, int k, double hs) {
#pragma clang fp contract(off)
    const double d = (double)k * hs;
    return t0 + d;
}

// WIND: PLANT_CALM (the reference model: no sin, no wind arithmetic),
// PLANT_WIND (constant W0) or PLANT_GUST; hs: the RK4 substep length
template <int WIND>
__device__ __forceinline__ void plant_lane(const ModelConst& P, int i, const double* __restrict__ wind8,
                                           double* __restrict__ x13, const double* __restrict__ u4, double t0,
                                           double hs, int steps, int substeps, int32_t* __restrict__ status) {
    double x[NK], u[NKU];
#pragma unroll
    for (int j = 0; j < NK; ++j) x[j] = x13[(size_t)i * NK + j];
#pragma unroll
    for (int j = 0; j < NKU; ++j) u[j] = u4[(size_t)i * NU + j];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < NK; ++j) fin = fin && isfinite(x[j]);
    int32_t flag = 0;
    if (!fin) {
        flag = KITE_PLANT_NAN;                  // non-finite on entry: the row stays as it is
    } else {
        double W0[3] = {0.0, 0.0, 0.0}, A[3] = {0.0, 0.0, 0.0}, om = 0.0, ph = 0.0;
        if constexpr (WIND != PLANT_CALM) {
            const double* w = wind8 + (size_t)i * 8;
#pragma unroll
            for (int j = 0; j < 3; ++j) W0[j] = w[j];
            if constexpr (WIND == PLANT_GUST) {
#pragma unroll
                for (int j = 0; j < 3; ++j) A[j] = w[3 + j];
                om = 2.0 * M_PI * w[6];
                ph = w[7];
            }
        }
        int k = 0;
        bool alive = true;
        for (int s = 0; s < steps && alive; ++s) {
            for (int m = 0; m < substeps; ++m, ++k) {
                const double t = plant_time(t0, k, hs);
                double xs[NK], acc[NK], kv[NK];
#pragma unroll
                for (int j = 0; j < NK; ++j) { xs[j] = x[j]; acc[j] = x[j]; }
#pragma unroll 1
                for (int st = 0; st < 4; ++st) {
                    double wnd[3] = {W0[0], W0[1], W0[2]};
                    if constexpr (WIND == PLANT_GUST) {
                        const double ts = st == 0 ? t : (st == 3 ? t + hs : t + 0.5 * hs);
                        const double sn = sin(om * ts + ph);
#pragma unroll
                        for (int j = 0; j < 3; ++j) wnd[j] = W0[j] + A[j] * sn;
                    }
                    kite_rhs<double, WIND != PLANT_CALM>(P, xs, u, kv, wnd);
                    const double wa = (st == 0 || st == 3) ? hs / 6.0 : hs / 3.0;
                    const double wn = (st < 2) ? 0.5 * hs : hs;
#pragma unroll
                    for (int j = 0; j < NK; ++j) { acc[j] += wa * kv[j]; xs[j] = x[j] + wn * kv[j]; }
                }
                bool ok = true;
#pragma unroll
                for (int j = 0; j < NK; ++j) ok = ok && isfinite(acc[j]);
                if (!ok) {                      // keep the last finite state, skip the rest
                    flag = KITE_PLANT_NAN;
                    alive = false;
                    break;
                }
#pragma unroll
                for (int j = 0; j < NK; ++j) x[j] = acc[j];
            }
        }
#pragma unroll
        for (int j = 0; j < NK; ++j) x13[(size_t)i * NK + j] = x[j];
    }
    if (status) status[i] = flag;
}

// PERKITE: the lane's constants come from mcf ([field][kite]), 47 coalesced
// loads at kernel start that then live in registers next to the RK4 state;
// otherwise from the kernel argument, as k_predict takes them.  One wave per
// block and no occupancy request: the flagship batch (4096 kites) is 64 waves
// on 256 CUs, so a lane's latency is what counts and the register allocator
// gets the whole file rather than a cap that would spill the constants.
template <bool PERKITE, int WIND>
__global__ __launch_bounds__(64) void k_plant(ModelConst Pc, const double* __restrict__ mcf, int B,
                                              const double* __restrict__ wind8, double* __restrict__ x13,
                                              const double* __restrict__ u4, double t0, double hs, int steps,
                                              int substeps, int32_t* __restrict__ status) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B) return;
    if constexpr (PERKITE) {
        double pf[kModelConstDoubles];
#pragma unroll
        for (int f = 0; f < kModelConstDoubles; ++f) pf[f] = mcf[(size_t)f * B + i];
        ModelConst P;
        __builtin_memcpy(&P, pf, sizeof(P));
        plant_lane<WIND>(P, i, wind8, x13, u4, t0, hs, steps, substeps, status);
    } else {
        plant_lane<WIND>(Pc, i, wind8, x13, u4, t0, hs, steps, substeps, status);
    }
}

hipError_t launch_plant(const ModelConst& P, const double* mcf, int B, int wind_mode, const double* wind8,
                        double* x13, const double* u4, double t0, double hs, int steps, int substeps,
                        int32_t* status, hipStream_t s) {
    const dim3 grid((B + 63) / 64), block(64);
#define KITE_PLANT_LAUNCH(PK, WM) \
    hipLaunchKernelGGL((k_plant<PK, WM>), grid, block, 0, s, P, mcf, B, wind8, x13, u4, t0, hs, steps, substeps, status)
    if (mcf) {
        if (wind_mode == PLANT_GUST) KITE_PLANT_LAUNCH(true, PLANT_GUST);
        else if (wind_mode == PLANT_WIND) KITE_PLANT_LAUNCH(true, PLANT_WIND);
        else KITE_PLANT_LAUNCH(true, PLANT_CALM);
    } else {
        if (wind_mode == PLANT_GUST) KITE_PLANT_LAUNCH(false, PLANT_GUST);
        else if (wind_mode == PLANT_WIND) KITE_PLANT_LAUNCH(false, PLANT_WIND);
        else KITE_PLANT_LAUNCH(false, PLANT_CALM);
    }
#undef KITE_PLANT_LAUNCH
    return hipGetLastError();
}

}  // namespace kite
