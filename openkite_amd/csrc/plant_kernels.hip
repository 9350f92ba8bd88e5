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
// not the plant's.  k_plant_delay (below) is the same plant behind a command
// line per kite: the reference's transport delay, still one launch per period.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "delay_line.hpp"
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

// What stands between the command and the plant.  NoLine: nothing, the held
// u4 flies (k_plant).  DelayLine: the kite's command line (k_plant_delay,
// below): L its KITE_DELAY_NLINE doubles in memory, n the pending commands
// after the send, head those that have left the FIFO in this call, flag the
// send's KITE_PLANT_* bits.
struct NoLine {
    static constexpr bool kDelay = false;
};
struct DelayLine {
    static constexpr bool kDelay = true;
    double* L;
    int n, head;
    int32_t flag;
};

// a plant tick at time tj: every pending command with t_arr <= tj leaves the
// FIFO in order, the last of them is the control in force from here on.  The
// head's arrival time is re-read from the line (one load per tick)
__device__ __forceinline__ void delay_arrivals(DelayLine& ln, double tj, double (&u)[NKU]) {
    while (ln.head < ln.n && ln.L[KITE_DELAY_T_ARR + ln.head] <= tj) {
#pragma unroll
        for (int j = 0; j < NKU; ++j) u[j] = ln.L[KITE_DELAY_U + NU * ln.head + j];
        ++ln.head;
    }
}

// WIND: PLANT_CALM (the reference model: no sin, no wind arithmetic),
// PLANT_WIND (constant W0) or PLANT_GUST; hs: the RK4 substep length.
// LINE: NoLine or DelayLine.  Both kernels share this one function, the RK4
// substep with it; every line-specific statement sits under if constexpr, so
// that k_plant's instances are the code they were before the line existed
template <int WIND, class LINE>
__device__ __forceinline__ void plant_lane(const ModelConst& P, int i, const double* __restrict__ wind8,
                                           double* __restrict__ x13, const double* __restrict__ u4, double t0,
                                           double hs, int steps, int substeps, int32_t* __restrict__ status,
                                           LINE& ln) {
    double x[NK], u[NKU];
#pragma unroll
    for (int j = 0; j < NK; ++j) x[j] = x13[(size_t)i * NK + j];
    if constexpr (LINE::kDelay) {
#pragma unroll
        for (int j = 0; j < NKU; ++j) u[j] = ln.L[KITE_DELAY_U_FORCE + j];
    } else {
#pragma unroll
        for (int j = 0; j < NKU; ++j) u[j] = u4[(size_t)i * NU + j];
    }
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
            if constexpr (LINE::kDelay) delay_arrivals(ln, plant_time(t0, k, hs), u);
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
    if constexpr (LINE::kDelay) flag |= ln.flag;
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
        NoLine nl;
        plant_lane<WIND>(P, i, wind8, x13, u4, t0, hs, steps, substeps, status, nl);
    } else {
        NoLine nl;
        plant_lane<WIND>(Pc, i, wind8, x13, u4, t0, hs, steps, substeps, status, nl);
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

// ---- the plant behind a command line (transport_delay.cpp, simulator.cpp) ----
// Every kite owns a line of KITE_DELAY_NLINE doubles (kite_nmpc.h, KITE_DELAY_*):
// the control in force and a FIFO of at most KITE_DELAY_DEPTH commands with
// their arrival times.  One call is one control period: the command (if any) is
// sent, then before every plant step the commands that have arrived leave the
// FIFO in order and the last of them becomes the control in force.  The queue
// logic does not look at the kite's state, so a frozen kite's line goes on.
//
// The FIFO stays in memory.  The lane appends the sent command to its own row,
// re-reads the head's arrival time at each tick (one load, an L1/L2 hit; three
// per launch at the driver's shape) and loads a command's three controls when it
// arrives; the row is compacted at exit, when the RK4 registers are dead.  What
// the flight loop carries beyond k_plant's registers is two counters.
static_assert(NU == kLineNU, "the line's layout (delay_line.hpp)");

// the send (delay_line.hpp: delay_send) appends the command under the line's
// arrival rule, slot KITE_DELAY_RULE: sequential, t_arr = max(t_send,
// t_arr_prev) + tau, or transport, t_arr = max(t_send + tau, t_arr_prev).  The
// rule is the line's, so one launch may mix both

// the line at the call's end.  What has left the FIFO by the last tick does
// not depend on the flight (a frozen kite's line goes on): the pops the flight
// did not get to are made up here.  Then the last arrival becomes the control
// in force, the rest moves to the front and vacated slots are zeroed (the
// rule slot is not touched: the line keeps its rule).  The
// whole row comes into registers with one round of loads (the RK4 registers
// are dead by now) and the new row is selected with compares, not indexed: a
// chain of dependent loads and stores per slot costs more than the flight's
// ticks together
__device__ __forceinline__ void delay_finish(DelayLine& ln, double t_last, double* __restrict__ u_applied, int i) {
    double* L = ln.L;
    double ta[KITE_DELAY_DEPTH], uq[KITE_DELAY_DEPTH][NU], uf[NU];
#pragma unroll
    for (int s = 0; s < KITE_DELAY_DEPTH; ++s) {
        ta[s] = L[KITE_DELAY_T_ARR + s];
#pragma unroll
        for (int q = 0; q < NU; ++q) uq[s][q] = L[KITE_DELAY_U + NU * s + q];
    }
#pragma unroll
    for (int q = 0; q < NU; ++q) uf[q] = L[KITE_DELAY_U_FORCE + q];
    const int n = ln.n;
    int head = ln.head;
#pragma unroll
    for (int s = 0; s < KITE_DELAY_DEPTH; ++s)      // in order: slot s leaves only once every slot before it has
        if (head == s && s < n && ta[s] <= t_last) head = s + 1;
    ln.head = head;
#pragma unroll
    for (int s = 0; s < KITE_DELAY_DEPTH; ++s) {
        if (head == s + 1) {
#pragma unroll
            for (int q = 0; q < NU; ++q) uf[q] = uq[s][q];
        }
    }
#pragma unroll
    for (int s = 0; s < KITE_DELAY_DEPTH; ++s) {    // slot s <- slot s + head if that is pending, else zero
        double t = 0.0, v[NU] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int src = s; src < KITE_DELAY_DEPTH; ++src) {
            if (src - s == head && src < n) {
                t = ta[src];
#pragma unroll
                for (int q = 0; q < NU; ++q) v[q] = uq[src][q];
            }
        }
        L[KITE_DELAY_T_ARR + s] = t;
#pragma unroll
        for (int q = 0; q < NU; ++q) L[KITE_DELAY_U + NU * s + q] = v[q];
    }
    L[KITE_DELAY_COUNT] = (double)(n - head);
#pragma unroll
    for (int q = 0; q < NU; ++q) L[KITE_DELAY_U_FORCE + q] = uf[q];
    if (u_applied) {
#pragma unroll
        for (int q = 0; q < NU; ++q) u_applied[(size_t)i * NU + q] = uf[q];
    }
}

// k_plant's six variants behind the line; the send runs before the constants
// are loaded, the flight as in k_plant
template <bool PERKITE, int WIND>
__global__ __launch_bounds__(64) void k_plant_delay(ModelConst Pc, const double* __restrict__ mcf, int B,
                                                    const double* __restrict__ wind8, double* __restrict__ x13,
                                                    const double* __restrict__ u_cmd, const double* __restrict__ tau,
                                                    double* line, double* __restrict__ u_applied, double t0,
                                                    double hs, int steps, int substeps, int32_t* __restrict__ status) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= B) return;
    DelayLine ln;
    ln.L = line + (size_t)i * KITE_DELAY_NLINE;
    ln.head = 0;
    ln.flag = 0;
    ln.n = delay_send(ln.L, u_cmd, tau, i, t0, ln.flag);
    const double t_last = plant_time(t0, (steps - 1) * substeps, hs);
    if constexpr (PERKITE) {
        double pf[kModelConstDoubles];
#pragma unroll
        for (int f = 0; f < kModelConstDoubles; ++f) pf[f] = mcf[(size_t)f * B + i];
        ModelConst P;
        __builtin_memcpy(&P, pf, sizeof(P));
        plant_lane<WIND>(P, i, wind8, x13, nullptr, t0, hs, steps, substeps, status, ln);
    } else {
        plant_lane<WIND>(Pc, i, wind8, x13, nullptr, t0, hs, steps, substeps, status, ln);
    }
    delay_finish(ln, t_last, u_applied, i);
}

hipError_t launch_plant_delay(const ModelConst& P, const double* mcf, int B, int wind_mode, const double* wind8,
                              double* x13, const double* u_cmd, const double* tau, double* line, double* u_applied,
                              double t0, double hs, int steps, int substeps, int32_t* status, hipStream_t s) {
    const dim3 grid((B + 63) / 64), block(64);
#define KITE_PLANT_LAUNCH(PK, WM)                                                                               \
    hipLaunchKernelGGL((k_plant_delay<PK, WM>), grid, block, 0, s, P, mcf, B, wind8, x13, u_cmd, tau, line, \
                       u_applied, t0, hs, steps, substeps, status)
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
