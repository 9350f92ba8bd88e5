// score_kernels.hip -- closed-loop scoring on the device (gfx950).
//
// One kite per wavefront of 64 lanes, four kites per 256-thread block.
//
// Closest point, global: lane j evaluates the path at theta_j = 2 pi j / 64; a
// wave reduction picks the nearest sample (the lowest j on a tie); every lane
// then runs the same safeguarded Newton iteration on g(theta) = (P - r) . P'
// from that sample, clamped to the sample's two neighbours.  The iteration is
// redundant across the lanes, so its result needs no broadcast, and every wave
// reduction sits in wave-uniform control flow.
//
// k_score: the closest point is its first phase; then lane 0 adds the period
// to the kite's accumulator row with plain fp64 adds.  A row depends on its own
// kite's inputs only: it is bitwise independent of the kite's place in the
// batch and of the batch size.  No atomics; every result is an ordinary
// vector store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rti_device.hpp"
#include "score_kernels.hpp"

namespace kite {

namespace {

constexpr int SCORE_WAVES = 4;                       // kites per block
constexpr double kTwoPi = 6.283185307179586476925;
constexpr double kPi = 3.141592653589793238463;
constexpr double kSampleStep = kTwoPi / kScoreSamples;

__device__ __forceinline__ V3<double> score_rot(const ScoreConst& C, const double v[3]) {
    const double qw = C.pq[0];
    const V3<double> qu{C.pq[1], C.pq[2], C.pq[3]};
    const double ww_uu = qw * qw - dot3(qu, qu);
    return rot_body(qw, qu, ww_uu, V3<double>{v[0], v[1], v[2]});
}

// P(theta) alone (the sampling phase)
__device__ __forceinline__ V3<double> score_path(const ScoreConst& C, double th) {
    double s, c;
    sincos(th, &s, &c);
    double p[3], dp[3];
    path_curve(C.path_K, C.path_R, C.path_alt, C.pF, c, s, p, dp);
    return score_rot(C, p);
}

// P, P' and P'' at theta
__device__ __forceinline__ void score_path2(const ScoreConst& C, double th, V3<double>& P, V3<double>& dP,
                                            V3<double>& ddP) {
    double s, c;
    sincos(th, &s, &c);
    double p[3], dp[3], ddp[3];
    path_curve(C.path_K, C.path_R, C.path_alt, C.pF, c, s, p, dp);
    path_curve2(C.path_K, C.path_R, C.pF, c, s, ddp);
    P = score_rot(C, p);
    dP = score_rot(C, dp);
    ddP = score_rot(C, ddp);
}

// Global closest point of the path to r, by one wavefront (all 64 lanes, in
// wave-uniform control flow).  Returns theta* in [-2 pi / 64, 2 pi) in every
// lane, the offset E = P(theta*) - r and d = ||E||; a non-finite r gives NaN.
__device__ __forceinline__ double closest_global(const ScoreConst& C, int lane, const V3<double>& r, V3<double>& E,
                                                 double& d) {
    const V3<double> Pj = score_path(C, (double)lane * kSampleStep);
    const V3<double> ej{Pj.x - r.x, Pj.y - r.y, Pj.z - r.z};
    const double d2 = dot3(ej, ej);
    const double m = wave_min(d2);
    // the lowest lane that holds the minimum (lane numbers are exact in fp64)
    const int jmin = (int)wave_min(d2 == m ? (double)lane : (double)kScoreSamples);
    const bool finite = isfinite(r.x) && isfinite(r.y) && isfinite(r.z);
    double th = (double)jmin * kSampleStep;
    const double lo = th - kSampleStep, hi = th + kSampleStep;
    V3<double> P, dP, ddP;
    for (int it = 0; it < kScoreNewton; ++it) {
        score_path2(C, th, P, dP, ddP);
        const V3<double> e{P.x - r.x, P.y - r.y, P.z - r.z};
        const double g = dot3(e, dP);
        const double gn = dot3(dP, dP);
        double h = gn + dot3(e, ddP);
        if (h <= 0.0) h = gn;
        if (!(h > 0.0)) break;                      // a stationary point of the curve, or NaN
        double tn = th - g / h;
        tn = tn < lo ? lo : (tn > hi ? hi : tn);
        if (tn == th) break;
        th = tn;
    }
    P = score_path(C, th);
    E = V3<double>{P.x - r.x, P.y - r.y, P.z - r.z};
    d = sqrt(dot3(E, E));
    if (!finite) { th = NAN; d = NAN; }
    return th;
}

}  // namespace

__global__ __launch_bounds__(64 * SCORE_WAVES) void k_closest_global(ScoreConst C, int count,
                                                                    const double* __restrict__ pos,
                                                                    double* __restrict__ theta,
                                                                    double* __restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * SCORE_WAVES + (threadIdx.x >> 6);
    if (b >= count) return;                          // the whole wave leaves
    const double* p = pos + (size_t)b * 3;
    const V3<double> r{p[0], p[1], p[2]};
    V3<double> E;
    double d;
    const double th = closest_global(C, lane, r, E, d);
    if (lane == 0) { theta[b] = th; dist[b] = d; }
}

__global__ __launch_bounds__(64 * SCORE_WAVES) void k_score(ScoreConst C, int count, const double* __restrict__ x13,
                                                           const double* __restrict__ u4,
                                                           const int32_t* __restrict__ status,
                                                           const int32_t* __restrict__ plant_status, int first,
                                                           double* __restrict__ acc, double* __restrict__ mem) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * SCORE_WAVES + (threadIdx.x >> 6);
    if (b >= count) return;                          // the whole wave leaves
    const double* x = x13 + (size_t)b * 13;
    const double* u = u4 + (size_t)b * 4;
    // lanes 0-12 look at one state each, lanes 13-16 at one control each
    double mine = 0.0;
    if (lane < 13) mine = x[lane];
    else if (lane < 17) mine = u[lane - 13];
    const int bad_in = wave_or(isfinite(mine) ? 0 : 1);
    const V3<double> r{x[6], x[7], x[8]};
    V3<double> E;
    double d;
    const double th = closest_global(C, lane, r, E, d);
    // ---- no wave reduction below this line ----
    if (lane != 0) return;
    const int st = status ? status[b] : 0;
    const int ps = plant_status ? plant_status[b] : 0;
    double* A = acc + (size_t)b * kScoreNacc;
    double* M = mem + (size_t)b * kScoreNmem;
    const double u0 = u[0], u1 = u[1], u2 = u[2], u3 = u[3];
    const double e0 = C.Sr[0] * E.x, e1 = C.Sr[1] * E.y, e2 = C.Sr[2] * E.z;
    const double ltrack = C.Q[0] * (e0 * e0) + C.Q[1] * (e1 * e1) + C.Q[2] * (e2 * e2);
    const double s0 = C.Su[0] * u0, s1 = C.Su[1] * u1, s2 = C.Su[2] * u2, s3 = C.Su[3] * u3;
    const double lu = C.R[0] * (s0 * s0) + C.R[1] * (s1 * s1) + C.R[2] * (s2 * s2) + C.R[3] * (s3 * s3);
    const double speed = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    // lost: the plant froze the kite, the data is non-finite, the controller
    // applied no fresh plan; or a finite input overflows a scored quantity
    const bool lost = bad_in || (ps & kPlantNan) || (st & (kStNan | kStStepRejected | kStRestart)) ||
                      !(isfinite(d * d) && isfinite(ltrack) && isfinite(lu) && isfinite(speed));
    if (lost) {
        A[kScoreNLost] += 1.0;
        A[kScoreEverLost] = 1.0;
        M[kScoreMemValid] = 0.0;
        return;
    }
    const double n = A[kScoreN];
    A[kScoreN] = n + 1.0;
    A[kScoreSumD2] += d * d;
    A[kScoreMaxD] = n == 0.0 ? d : fmax(A[kScoreMaxD], d);
    A[kScoreSumTrack] += ltrack;
    A[kScoreSumU] += lu;
    A[kScoreSumSpeed] += speed;
    A[kScoreMinSpeed] = n == 0.0 ? speed : fmin(A[kScoreMinSpeed], speed);
    if (!first && M[kScoreMemValid] != 0.0) {
        const double r0 = C.Su[0] * (u0 - M[kScoreMemU + 0]), r1 = C.Su[1] * (u1 - M[kScoreMemU + 1]);
        const double r2 = C.Su[2] * (u2 - M[kScoreMemU + 2]), r3 = C.Su[3] * (u3 - M[kScoreMemU + 3]);
        A[kScoreSumRate] += r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3;
        double dth = th - M[kScoreMemTheta];         // wrap to (-pi, pi]
        if (dth > kPi) dth -= kTwoPi;
        else if (dth <= -kPi) dth += kTwoPi;
        A[kScoreProgress] += dth;
        A[kScoreNRate] += 1.0;
    }
    if (st & kStMinSpeed) A[kScoreNMinSpeed] += 1.0;
    if (st & kStQpNotConv) A[kScoreNQpNotConv] += 1.0;
    if (st & kStStateBound) A[kScoreNStateBound] += 1.0;
    M[kScoreMemTheta] = th;
    M[kScoreMemU + 0] = u0; M[kScoreMemU + 1] = u1; M[kScoreMemU + 2] = u2; M[kScoreMemU + 3] = u3;
    M[kScoreMemValid] = 1.0;
}

// Fleet summary: one block.  Thread t reduces rows t, t + 256, ... in index
// order, then a fixed LDS tree combines the 256 partial rows: the order of
// every operation is a function of `count` alone, so two launches agree bit
// for bit.
constexpr int SUM_T = 256;
__global__ __launch_bounds__(SUM_T) void k_score_summary(int count, const double* __restrict__ acc,
                                                        double* __restrict__ out) {
    __shared__ double sh[kScoreNsum][SUM_T];
    const int t = threadIdx.x;
    double v[kScoreNsum];
#pragma unroll
    for (int k = 0; k < kScoreNsum; ++k) v[k] = 0.0;
    double any = 0.0;                                // a row with n > 0 went into max / min
    for (int b = t; b < count; b += SUM_T) {
        const double* A = acc + (size_t)b * kScoreNacc;
        const double n = A[kScoreN];
#pragma unroll
        for (int k = 0; k < kScoreNacc; ++k) {
            if (k == kScoreMaxD || k == kScoreMinSpeed || k == kScoreKites) continue;
            v[k] += A[k];
        }
        v[kScoreKites] += 1.0;
        if (n > 0.0) {
            v[kScoreMaxD] = any != 0.0 ? fmax(v[kScoreMaxD], A[kScoreMaxD]) : A[kScoreMaxD];
            v[kScoreMinSpeed] = any != 0.0 ? fmin(v[kScoreMinSpeed], A[kScoreMinSpeed]) : A[kScoreMinSpeed];
            any = 1.0;
        }
    }
    // kScoreN of the partial row doubles as "this partial holds a max / min":
    // it is > 0 exactly when a row with n > 0 was reduced into it
#pragma unroll
    for (int k = 0; k < kScoreNsum; ++k) sh[k][t] = v[k];
    __syncthreads();
    for (int s = SUM_T / 2; s > 0; s >>= 1) {
        if (t < s) {
            const bool ha = sh[kScoreN][t] > 0.0, hb = sh[kScoreN][t + s] > 0.0;
#pragma unroll
            for (int k = 0; k < kScoreNsum; ++k) {
                if (k == kScoreN) continue;          // read above, combined last
                const double a = sh[k][t], c = sh[k][t + s];
                double o;
                if (k == kScoreMaxD) o = ha && hb ? fmax(a, c) : (hb ? c : a);
                else if (k == kScoreMinSpeed) o = ha && hb ? fmin(a, c) : (hb ? c : a);
                else o = a + c;
                sh[k][t] = o;
            }
            sh[kScoreN][t] += sh[kScoreN][t + s];
        }
        __syncthreads();
    }
    if (t < kScoreNsum) out[t] = sh[t][0];
}

hipError_t launch_closest_point_global(const ScoreConst& C, int count, const double* pos, double* theta,
                                       double* dist, hipStream_t s) {
    hipLaunchKernelGGL(k_closest_global, dim3((count + SCORE_WAVES - 1) / SCORE_WAVES), dim3(64 * SCORE_WAVES), 0, s,
                       C, count, pos, theta, dist);
    return hipGetLastError();
}

hipError_t launch_score(const ScoreConst& C, int count, const double* x13, const double* u4, const int32_t* status,
                        const int32_t* plant_status, int first, double* acc, double* mem, hipStream_t s) {
    hipLaunchKernelGGL(k_score, dim3((count + SCORE_WAVES - 1) / SCORE_WAVES), dim3(64 * SCORE_WAVES), 0, s, C,
                       count, x13, u4, status, plant_status, first, acc, mem);
    return hipGetLastError();
}

hipError_t launch_score_summary(int count, const double* acc, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_score_summary, dim3(1), dim3(SUM_T), 0, s, count, acc, out);
    return hipGetLastError();
}

}  // namespace kite
