// score_kernels.hpp -- internal interface between the C ABI (kite_nmpc.cpp) and
// the closed-loop scoring kernels (score_kernels.hip): the global closest point
// on the path, the per-period flight metrics of every kite and their fleet
// summary.  The slot layout of the accumulators is the public one
// (KITE_SCORE_* in include/kite_nmpc/kite_nmpc.h); it is restated here so the
// kernels need not see the C header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kite_path.hpp"

namespace kite {

// d2p/dtheta2 of the unrotated path curve (kite_path.hpp path_curve):
// p''_a = -sum_{k <= K} k^2 (F[a][2k-1] cos k theta + F[a][2k] sin k theta); the
// circle (K = 0): [-R cos, -R sin, 0].  c = cos(theta), s = sin(theta); the
// same angle-addition recurrence and the same compile-time coefficient indices
// as path_curve.
__host__ __device__ inline void path_curve2(int K, double R, const double (*F)[KITE_PATH_NC], double c, double s,
                                            double ddp[3]) {
    if (K == 0) {
        ddp[0] = -R * c; ddp[1] = -R * s; ddp[2] = 0.0;
        return;
    }
    for (int a = 0; a < 3; ++a) ddp[a] = 0.0;
    double ck = c, sk = s;
#pragma unroll
    for (int k = 1; k <= KITE_PATH_HMAX; ++k) {
        if (k > K) break;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double ak = F[a][2 * k - 1], bk = F[a][2 * k];
            ddp[a] -= (double)(k * k) * (ak * ck + bk * sk);
        }
        const double cn = ck * c - sk * s, sn = sk * c + ck * s;
        ck = cn; sk = sn;
    }
}

// Samples of the global closest-point search: one per lane of a wavefront.
constexpr int kScoreSamples = 64;
// Newton iterations after the sampling (8 reach the rounding floor on the
// node's circle and on a three-harmonic path; the loop stops when the iterate
// no longer changes).
constexpr int kScoreNewton = 12;

// ---- accumulator row of one kite (acc, B x kScoreNacc), KITE_SCORE_* --------
// An all-zero row is the reset state.  Slots 0-2 and 11-14 hold integers.
constexpr int kScoreNacc = 16;
constexpr int kScoreN = 0;            // scored periods
constexpr int kScoreNLost = 1;        // lost periods
constexpr int kScoreEverLost = 2;     // 1 once a period was lost
constexpr int kScoreSumD2 = 3;        // sum d^2 [m^2], d the true cross-track distance
constexpr int kScoreMaxD = 4;         // max d [m]               (valid when n > 0)
constexpr int kScoreSumTrack = 5;     // sum l_track, the controller's position cost at the closest point
constexpr int kScoreSumU = 6;         // sum l_u = sum_i R_i (Su_i u_i)^2
constexpr int kScoreSumRate = 7;      // sum ||Su (u - u_prev)||^2 over the periods that have a predecessor
constexpr int kScoreSumSpeed = 8;     // sum ||v_b|| [m/s]
constexpr int kScoreMinSpeed = 9;     // min ||v_b|| [m/s]       (valid when n > 0)
constexpr int kScoreProgress = 10;    // sum wrap(theta* - theta*_prev) [rad]; laps = progress / 2 pi
constexpr int kScoreNMinSpeed = 11;   // scored periods with KITE_ST_MIN_SPEED
constexpr int kScoreNQpNotConv = 12;  // scored periods with KITE_ST_QP_NOT_CONV
constexpr int kScoreNStateBound = 13; // scored periods with KITE_ST_STATE_BOUND
constexpr int kScoreNRate = 14;       // periods that contributed to the rate and the progress
constexpr int kScoreSpare = 15;       // 0
// the fleet summary (kScoreNsum doubles) holds the same slots reduced over the
// kites: sums, except max over kScoreMaxD and min over kScoreMinSpeed (both
// over the kites with n > 0; 0 when there is none), and the number of rows
// reduced in kScoreKites
constexpr int kScoreNsum = 16;
constexpr int kScoreKites = 15;

// ---- memory row of one kite (mem, B x kScoreNmem), KITE_SCORE_MEM_* ---------
constexpr int kScoreNmem = 8;
constexpr int kScoreMemTheta = 0;     // theta* of the last scored period
constexpr int kScoreMemU = 1;         // u4 of the last scored period (slots 1-4)
constexpr int kScoreMemValid = 5;     // 1: slots 0-4 are the period before this one; 0 after a lost period
                                      // (slots 6, 7 spare)

// status bits the scorer reads (KITE_ST_*, KITE_PLANT_NAN)
constexpr int kStNan = 1, kStQpNotConv = 2, kStMinSpeed = 4, kStStateBound = 8, kStStepRejected = 32, kStRestart = 64;
constexpr int kPlantNan = 1;

// Everything the scoring kernels need, from kite_nmpc_config (kernel argument).
struct ScoreConst {
    int path_K, pad_;
    double path_R, path_alt, pq[4];
    double Q[3], Sr[3];     // path weights, Sx[6..8]
    double R[4], Su[4];
    double pF[3][KITE_PATH_NC];
};

// theta (count), dist (count) of the global closest point to pos (count x 3)
hipError_t launch_closest_point_global(const ScoreConst& C, int count, const double* pos, double* theta,
                                       double* dist, hipStream_t s);
// one control period of `count` kites into acc (count x kScoreNacc) and mem
// (count x kScoreNmem); status, plant_status: count words each, nullable
hipError_t launch_score(const ScoreConst& C, int count, const double* x13, const double* u4, const int32_t* status,
                        const int32_t* plant_status, int first, double* acc, double* mem, hipStream_t s);
// out (kScoreNsum) from acc (count x kScoreNacc)
hipError_t launch_score_summary(int count, const double* acc, double* out, hipStream_t s);

}  // namespace kite
