// delay_line.hpp -- the per-kite command line as plain functions of a row of
// doubles: the send of k_plant_delay (plant_kernels.hip), the in-flight
// schedule row k_inflight builds from a line, and the substep rule of the
// queue-aware delay compensation (prologue_kite, rti_kernels.hip).  No state,
// no HIP call: the same text compiles for the device and, without hipcc, for
// the host (tests/cpp/delay_line_check.cpp runs it under the sanitizers
// against the Python models).
#pragma once
#include <cmath>
#include <stdint.h>

#include "kite_nmpc/kite_nmpc.h"

#if defined(__HIPCC__)
#define KITE_LINE_FN __host__ __device__ __forceinline__
#else
#define KITE_LINE_FN inline
#endif

namespace kite {

constexpr int kLineNU = 4;      // doubles per command in the line (T, dE, dR, 4th)
static_assert(KITE_DELAY_DEPTH == 4 && KITE_DELAY_NLINE == 32 && KITE_DELAY_U == KITE_DELAY_T_ARR + KITE_DELAY_DEPTH &&
              KITE_DELAY_U + kLineNU * KITE_DELAY_DEPTH <= KITE_DELAY_NLINE && KITE_DELAY_RULE == 3,
              "the line's layout");
static_assert(KITE_INFLIGHT_N >= 8 + 3 * KITE_DELAY_DEPTH, "the schedule row's layout");

// the pending count as the line's readers take it: 0 .. DEPTH, NaN: 0
KITE_LINE_FN int delay_count(const double* L) {
    const double c = L[KITE_DELAY_COUNT];
    return c >= 1.0 ? (c >= (double)KITE_DELAY_DEPTH ? KITE_DELAY_DEPTH : (int)c) : 0;
}

// the send.  Sequential rule: t_arr = max(t_send, t_arr_prev) + tau (the
// sequential sleep of TDelay::publish).  Transport rule (slot KITE_DELAY_RULE
// exactly 1.0): t_arr = max(t_send + tau, t_arr_prev), a pure transport delay
// with the FIFO clamp.  Under both the channel never reorders.  Returns the
// pending count
KITE_LINE_FN int delay_send(double* L, const double* __restrict__ u_cmd, const double* __restrict__ tau,
                            int i, double t0, int32_t& flag) {
    int n = delay_count(L);
    if (u_cmd) {
        const double ta = tau[i];
        if (!(ta >= 0.0) || !std::isfinite(ta)) {
            flag |= KITE_PLANT_BAD_TAU;         // the command is dropped
        } else {
            const bool transport = L[KITE_DELAY_RULE] == (double)KITE_DELAY_RULE_TRANSPORT;
            const double prev = L[KITE_DELAY_HAS_PREV] != 0.0 ? L[KITE_DELAY_T_PREV] : t0;
            const double t_arr = transport ? std::fmax(t0 + ta, prev) : std::fmax(t0, prev) + ta;
            if (n == KITE_DELAY_DEPTH) {        // full: the oldest goes (circular_buffer::push_back)
                for (int s = 0; s + 1 < KITE_DELAY_DEPTH; ++s) {
                    L[KITE_DELAY_T_ARR + s] = L[KITE_DELAY_T_ARR + s + 1];
                    for (int q = 0; q < kLineNU; ++q)
                        L[KITE_DELAY_U + kLineNU * s + q] = L[KITE_DELAY_U + kLineNU * (s + 1) + q];
                }
                n = KITE_DELAY_DEPTH - 1;
                flag |= KITE_PLANT_CMD_DROPPED;
            }
            L[KITE_DELAY_T_ARR + n] = t_arr;
            for (int q = 0; q < kLineNU; ++q) L[KITE_DELAY_U + kLineNU * n + q] = u_cmd[(size_t)i * kLineNU + q];
            ++n;
            L[KITE_DELAY_T_PREV] = t_arr;
            L[KITE_DELAY_HAS_PREV] = 1.0;
        }
    }
    return n;
}

// the schedule row (kite_nmpc.h, KITE_INFLIGHT_N) of line L seen at time t0
KITE_LINE_FN void inflight_row(const double* __restrict__ L, double t0, double* __restrict__ row) {
    const int n = delay_count(L);
    double r[KITE_INFLIGHT_N];
#pragma unroll
    for (int j = 0; j < KITE_INFLIGHT_N; ++j) r[j] = 0.0;
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        r[5 + q] = L[KITE_DELAY_U_FORCE + q];
        ok = ok && std::isfinite(r[5 + q]);
    }
    double run = 0.0;
#pragma unroll
    for (int s = 0; s < KITE_DELAY_DEPTH; ++s) {
        if (s < n) {
            const double ta = L[KITE_DELAY_T_ARR + s];
            ok = ok && std::isfinite(ta);
            run = std::fmax(run, std::fmax(ta - t0, 0.0));      // the FIFO pops in order
            r[1 + s] = run;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                r[8 + 3 * s + q] = L[KITE_DELAY_U + kLineNU * s + q];
                ok = ok && std::isfinite(r[8 + 3 * s + q]);
            }
        }
    }
    r[0] = (double)n;
#pragma unroll
    for (int j = 0; j < KITE_INFLIGHT_N; ++j) row[j] = ok ? r[j] : (j == 0 ? -1.0 : 0.0);
}

// RK4 substeps of a piece of length len of the compensation window: the
// smallest n in 1 .. steps with (double)n * h_max >= len, steps if there is none
KITE_LINE_FN int inflight_substeps(double len, double h_max, int steps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    int n = 1;
    while (n < steps && (double)n * h_max < len) ++n;
    return n;
}

}  // namespace kite
