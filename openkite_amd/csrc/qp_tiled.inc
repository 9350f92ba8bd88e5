// qp_tiled.inc -- wave-per-instance interior-point QP on fp64 MFMA tiles
// (included by rti_kernels.hip inside namespace kite; N == 20 path).
//
// Same algorithm as k_qp (Mehrotra predictor-corrector, cold start, relative
// freeze, cap K, see oracle/kite_oracle.cpp qp_ipm), different linear algebra:
//
//   variables  w = [w_a (80: T,dE,dR x 20 | Uv x 20) | w_b (theta0, thetadot0)]
//   normal matrix  M = H + Sigma_box + C' Sigma_c C  with the C rows (vx) on w_a
//   M_aa (80 x 80) = 5 x 5 tiles of 16 x 16, the 15 lower tiles held in
//       registers in the v_mfma_f64_16x16x4_f64 C/D layout
//       (lane l: column l&15, rows (l>>4) + 4r, r = 0..3)
//   H_aa + C' Sigma_c C : copy of the H tiles + MFMA rank-20 update
//   Cholesky M_aa = L L' : right-looking blocked, diagonal tile by an
//       in-register 16-step Cholesky that also produces T_KK = L_KK^-1,
//       panel Y_I = T_KK M_IK' = L_IK' and trailing M_IJ -= L_IK L_JK' on
//       MFMA, the trailing operands straight from the Y_I registers
//   theta block by a 2 x 2 Schur complement S = M_bb - Y'Y, Y = L^-1 M_ab
//   solves: register-resident tile sweeps.  a-block vectors live in two
//       layouts: "col" (lane holds element 16K + cl of tile K, the same in
//       the 4 row-groups) and "row" (lane holds elements 16K + rg + 4r, the
//       same in the 16 lanes of a row).  L y = r maps row -> col, L' x = y
//       maps col -> row; reductions are DPP row sums and permlane column
//       sums -- no LDS traffic and no barrier inside a sweep.
// One wavefront per instance, 1 wave/SIMD, ~36 KB LDS.

// Optional phase profile (-DKITE_QP_PROF, tools only): shader-clock cycles per
// phase summed over all instances into g_qp_prof.
#ifdef KITE_QP_PROF
__device__ unsigned long long g_qp_prof[24];
#define QP_MARK(ph)                                                                  \
    do {                                                                             \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                  \
        prof_acc[ph] += t_ - prof_last;                                              \
        prof_last = t_;                                                              \
    } while (0)
#define QP_SUB(ph)                                                                   \
    do {                                                                             \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                  \
        sub[ph] += t_ - sub_t;                                                       \
        sub_t = t_;                                                                  \
    } while (0)
// load-wait sub-markers of k_qp_tiled (g_qp_prof[16..21]): QP_WSUB closes a
// segment; QP_WDRAIN first waits for every outstanding global load, so the
// segment it closes is the exposed load wait at that point (the product build
// waits there or at the first use a few instructions later)
#define QP_WSUB(ph)                                                                  \
    do {                                                                             \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                  \
        prof_wsub[ph] += t_ - prof_wt;                                               \
        prof_wt = t_;                                                                \
    } while (0)
#define QP_WSTART() do { prof_wt = __builtin_amdgcn_s_memtime(); } while (0)
#define QP_WDRAIN(ph)                                                                \
    do {                                                                             \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             \
        QP_WSUB(ph);                                                                 \
    } while (0)
// sums of a finished instance; `done` = 0 for a first phase that hands its kite
// on (the resumed instance counts the kite and all its iterations)
#define QP_PROF_FLUSH(done)                                                          \
    do {                                                                             \
        if (l == 0) {                                                                \
            for (int i = 0; i < 9; ++i) atomicAdd(&g_qp_prof[i], prof_acc[i]);       \
            if (done) {                                                              \
                atomicAdd(&g_qp_prof[9], (unsigned long long)iters);                 \
                atomicAdd(&g_qp_prof[10], 1ull);                                     \
            }                                                                        \
            for (int i = 0; i < 3; ++i) atomicAdd(&g_qp_prof[11 + i], prof_sub[i]);  \
            for (int i = 0; i < 6; ++i) atomicAdd(&g_qp_prof[16 + i], prof_wsub[i]); \
        }                                                                            \
    } while (0)
#else
#define QP_PROF_FLUSH(done) do { } while (0)
#define QP_MARK(ph) do { } while (0)
#define QP_SUB(ph) do { } while (0)
#define QP_WSUB(ph) do { } while (0)
#define QP_WSTART() do { } while (0)
#define QP_WDRAIN(ph) do { } while (0)
#endif

constexpr int TLD = 17;        // LDS row stride of a 16 x 16 tile: conflict-free rows and columns
constexpr int QNA = 16 * QP_NTA;   // 80
constexpr int QN = 4 * QP_NTA;     // horizon of the tiled path (N = 20)
constexpr int QNC = 64;            // columns kept of the vx-bound rows C (kite controls 3N = 60 < 64)
static_assert(QNC == 64, "one C column per lane");

__device__ __forceinline__ constexpr int TI(int I, int J) { return I * (I + 1) / 2 + J; }

// In-register Cholesky of a symmetric 16 x 16 tile `a` (C layout) that
// produces x = L^-1 (a is consumed; L itself is never needed: the panels and
// the sweeps use T = L^-1 only).  Blocked by register: register r holds rows
// 4r..4r+3, so pivot block PB is register PB.
//   1. the 4 rows of the block (a and x) are broadcast to every row-group by
//      three permlane swaps each (lane (rg, cl) then holds R[q] = A[4PB+q][cl]),
//   2. the 4 pivots are eliminated on these replicated rows with row_newbcast
//      DPP only (pivot, multipliers) -- U = L' rows and the X rows of the block,
//   3. the rows below the block get the rank-4 update on MFMA:
//      A -= U_blk' U_blk and X -= U_blk' X_blk (U_blk masked to columns past
//      the block, so the rows of finished blocks receive exact zeros).
// Same formulas as the row-by-row form: pivot safeguard, 1/sqrt by v_rsq_f64
// + 2 Newton steps, multiplier = U[P][i].
__device__ __forceinline__ void bcast_rows4(double v, double R[4]) {
    double ev, od;
    swap16_d(v, ev, od);           // rows {0|2}, {1|3} of this half
    swap32_d(ev, R[0], R[2]);
    swap32_d(od, R[1], R[3]);
}
template <int PB, int Q, int q>                                      // eliminate pivot 4PB+Q from row 4PB+q
__device__ __forceinline__ void chol_elim(double R[4], double XR[4]) {
    const double m = dpp_d<0x150 + 4 * PB + q>(R[Q]);                   // L[4PB+q][P] = U[P][4PB+q]
    R[q] = fma(-m, R[Q], R[q]);
    XR[q] = fma(-m, XR[Q], XR[q]);
    if constexpr (q < 3) chol_elim<PB, Q, q + 1>(R, XR);
}
template <int PB, int Q>
__device__ __forceinline__ void chol_piv(double R[4], double XR[4]) {
    constexpr int P = 4 * PB + Q;
    const double piv = dpp_d<0x150 + P>(R[Q]);                          // A[P][P] to every lane
    // pivot safeguard on the result: a pivot <= 0 (rounding near
    // convergence) gives a NaN from the rsq and its correction (0 * inf for a
    // zero pivot), which v_max_f64 turns into 0 -- the direction is frozen for
    // the step, as with the oracle's 1e128 pivot (1/sqrt = 1e-64; DESIGN 4.3);
    // a NaN row stays NaN through R[Q] * 0.  One VALU op instead of a compare
    // and two selects.
    const double inv = fmax(fast_rsq(piv), 0.0);
    R[Q] *= inv;                                                        // U[P][cl] (cl >= P)
    XR[Q] *= inv;
    if constexpr (Q < 3) {
        chol_elim<PB, Q, Q + 1>(R, XR);
        chol_piv<PB, Q + 1>(R, XR);
    }
}
template <int PB>
__device__ __forceinline__ void chol_block(double4v& a, double4v& x, int cl, int rg) {
    double R[4], XR[4];
    bcast_rows4(a[PB], R);
    if constexpr (PB == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) XR[q] = cl == q ? 1.0 : 0.0;   // rows 0..3 of x = I, no broadcast needed
    } else {
        bcast_rows4(x[PB], XR);
    }
    chol_piv<PB, 0>(R, XR);
    a[PB] = rg == 0 ? R[0] : rg == 1 ? R[1] : rg == 2 ? R[2] : R[3];
    x[PB] = rg == 0 ? XR[0] : rg == 1 ? XR[1] : rg == 2 ? XR[2] : XR[3];
    if constexpr (PB < 3) {
        const double fr = cl > 4 * PB + 3 ? a[PB] : 0.0;                // U_blk[k][cl], columns past the block
        x = __builtin_amdgcn_mfma_f64_16x16x4f64(-fr, x[PB], x, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f64_16x16x4f64(-fr, fr, a, 0, 0, 0);
        chol_block<PB + 1>(a, x, cl, rg);
    }
}

// a: symmetric 16 x 16 tile (C layout) -> x = L^-1 (a is consumed)
__device__ __forceinline__ void chol_tile(double4v& a, double4v& x, int l) {
    const int cl = l & 15, rg = l >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = (rg + 4 * r == cl) ? 1.0 : 0.0;
    chol_block<0>(a, x, cl, rg);
}

__device__ __forceinline__ void tile_store(double* dst, const double4v& a, int l) {
    const int cl = l & 15, rg = l >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(rg + 4 * r) * TLD + cl] = a[r];
}
// MFMA A/B fragment (k-step s) of a row-major LDS tile T: T[l&15][4s + (l>>4)]
__device__ __forceinline__ double tile_frag(const double* src, int s, int l) {
    return src[(l & 15) * TLD + 4 * s + (l >> 4)];
}

// blocked Cholesky of the 5 x 5 tile matrix in Mt (lower tiles); T_KK -> sT.
// Per step K the panel tiles M_IK are staged in sP and each panel is formed
// transposed on MFMA, Y_I = T_KK M_IK' = L_IK' (L_IK itself, C layout, goes to
// Mt for the sweeps through one LDS transpose off the critical path).  In C layout register r of Y_I holds
// L_IK[cl][rg + 4r], which is exactly the A operand (and Y_J the B operand) of
// k-step r of L_IK L_JK' when k-step r takes the k indices rg + 4r: the
// trailing update reads its operands from registers, with no LDS round trip
// and no barrier between the panels and the next diagonal tile.  The update
// of the diagonal tile K+1 (the next step's critical path) goes first, then
// its factorization, then the rest of the update.
__device__ __forceinline__ void chol_tiles(double4v* Mt, double* sT, double* sP, int l
#ifdef KITE_QP_PROF
                                           , unsigned long long* sub
#endif
                                           ) {
#ifdef KITE_QP_PROF
    unsigned long long sub_t = __builtin_amdgcn_s_memtime();
#endif
    double4v X;
    chol_tile(Mt[TI(0, 0)], X, l);
#pragma unroll
    for (int K = 0; K < QP_NTA; ++K) {
        tile_store(sT + K * 16 * TLD, X, l);
        if (K == QP_NTA - 1) break;
#pragma unroll
        for (int I = K + 1; I < QP_NTA; ++I) tile_store(sP + (I - K - 1) * 16 * TLD, Mt[TI(I, K)], l);
        wave_sync();
        QP_SUB(0);
        double4v Y[QP_NTA - 1];
#pragma unroll
        for (int I = K + 1; I < QP_NTA; ++I) {          // Y_I = T_KK M_IK' = L_IK'
            double4v yt = double4v{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4; ++s)
                yt = __builtin_amdgcn_mfma_f64_16x16x4f64(tile_frag(sT + K * 16 * TLD, s, l),
                                                          tile_frag(sP + (I - K - 1) * 16 * TLD, s, l), yt, 0, 0, 0);
            Y[I - K - 1] = yt;
        }
        QP_SUB(1);
#pragma unroll
        for (int r = 0; r < 4; ++r)                    // M_IJ -= L_IK L_JK', k-step r = Y_I[r], Y_J[r]
            Mt[TI(K + 1, K + 1)] = __builtin_amdgcn_mfma_f64_16x16x4f64(-Y[0][r], Y[0][r], Mt[TI(K + 1, K + 1)],
                                                                      0, 0, 0);
        chol_tile(Mt[TI(K + 1, K + 1)], X, l);
#pragma unroll
        for (int I = K + 2; I < QP_NTA; ++I)           // the rest of tile column K + 1
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Mt[TI(I, K + 1)] = __builtin_amdgcn_mfma_f64_16x16x4f64(-Y[I - K - 1][r], Y[0][r], Mt[TI(I, K + 1)],
                                                                        0, 0, 0);
#pragma unroll
        for (int J = K + 2; J < QP_NTA; ++J)
#pragma unroll
            for (int I = J; I < QP_NTA; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Mt[TI(I, J)] = __builtin_amdgcn_mfma_f64_16x16x4f64(-Y[I - K - 1][r], Y[J - K - 1][r],
                                                                        Mt[TI(I, J)], 0, 0, 0);
        wave_sync();                                   // staged reads done before Y overwrites them
#pragma unroll
        for (int I = K + 1; I < QP_NTA; ++I) tile_store(sP + (I - K - 1) * 16 * TLD, Y[I - K - 1], l);
        wave_sync();
#pragma unroll
        for (int I = K + 1; I < QP_NTA; ++I)           // L_IK = Y_I' (C layout) for the sweeps
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Mt[TI(I, K)][r] = sP[(I - K - 1) * 16 * TLD + (l & 15) * TLD + (l >> 4) + 4 * r];
        QP_SUB(2);
    }
}

// 1/d: hardware estimate + 2 Newton steps (step-length ratios only)
__device__ __forceinline__ double rcp_d(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(r, fma(-d, r, 1.0), r);
    return fma(r, fma(-d, r, 1.0), r);
}

// T_KK[cl][rg + 4r] from the row-major LDS tiles (tl = sT + cl * TLD + rg)
#define KITE_TL(K, r) tl[(K) * 16 * TLD + 4 * (r)]

// Row sums of the sweeps are taken four at a time (row_sum16x4, the four
// registers of one tile row); hi8 / hi4: bits 3 / 2 of the lane's column cl.

// L y = E r : r (b) and E (e) in LDS, formed per tile in row layout; y out in
// col layout (the right-hand side never occupies registers as a whole)
__device__ __forceinline__ void fwd_solve(const double4v* Mt, const double* tl, const double* b, const double* e,
                                          int rg, bool hi8, bool hi4, double y[QP_NTA]) {
#pragma unroll
    for (int K = 0; K < QP_NTA; ++K) {
        double p[4] = {0.0, 0.0, 0.0, 0.0};
        if (K > 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int J = 0; J < K; ++J) p[r] = fma(Mt[TI(K, J)][r], y[J], p[r]);   // L_KJ[rg+4r][cl] y_J[cl]
            row_sum16x4(p, hi8, hi4);
        }
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * K + rg + 4 * r;
            const double sres = b[i] * e[i] - p[r];
            acc = fma(KITE_TL(K, r), sres, acc);                                          // T[cl][rg+4r] s[rg+4r]
        }
        y[K] = col_sum4(acc);
    }
}

// L Y = E M_ab for both theta columns in one sweep (Schur block): each L
// element is moved out of its AGPR once for both right-hand sides, the two
// dependent chains interleave, and the right-hand sides are formed per tile
// from LDS (b0 / b1: M_ab columns, e: equilibration, row layout)
__device__ __forceinline__ void fwd_solve2(const double4v* Mt, const double* tl, const double* b0,
                                           const double* b1, const double* e, int rg, bool hi8, bool hi4,
                                           double y0[QP_NTA], double y1[QP_NTA]) {
#pragma unroll
    for (int K = 0; K < QP_NTA; ++K) {
        double p0[4] = {0.0, 0.0, 0.0, 0.0}, p1[4] = {0.0, 0.0, 0.0, 0.0};
        if (K > 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int J = 0; J < K; ++J) {
                    const double lv = Mt[TI(K, J)][r];
                    p0[r] = fma(lv, y0[J], p0[r]);
                    p1[r] = fma(lv, y1[J], p1[r]);
                }
            row_sum16x4(p0, hi8, hi4);
            row_sum16x4(p1, hi8, hi4);
        }
        double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * K + rg + 4 * r;
            const double ei = e[i];
            const double t = KITE_TL(K, r);
            acc0 = fma(t, b0[i] * ei - p0[r], acc0);
            acc1 = fma(t, b1[i] * ei - p1[r], acc1);
        }
        y0[K] = col_sum4(acc0);
        y1[K] = col_sum4(acc1);
    }
}

// L' x = y : y in col layout, x out in row layout
__device__ __forceinline__ void bwd_solve(const double4v* Mt, const double* tl, const double y[QP_NTA], bool hi8,
                                          bool hi4, double x[QP_NTA][4]) {
#pragma unroll
    for (int K = QP_NTA - 1; K >= 0; --K) {
        double sres = y[K];
        if (K < QP_NTA - 1) {
            double p[4] = {0.0, 0.0, 0.0, 0.0};                 // four short chains instead of one long one
#pragma unroll
            for (int J = K + 1; J < QP_NTA; ++J)
#pragma unroll
                for (int r = 0; r < 4; ++r) p[r] = fma(Mt[TI(J, K)][r], x[J][r], p[r]);   // L_JK[rg+4r][cl] x_J[rg+4r]
            sres -= col_sum4((p[0] + p[1]) + (p[2] + p[3]));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) x[K][r] = KITE_TL(K, r) * sres;                      // T[cl][rg+4r] s[cl]
        row_sum16x4(x[K], hi8, hi4);                                                      // summed over cl
    }
}

// out = H_aa w (symmetric; lower tiles in registers, C layout); w, out in LDS
__device__ __forceinline__ void tile_symv(const double4v* Ht, const double* w, double* out, int l) {
    const int cl = l & 15, rg = l >> 4;
    double yr[QP_NTA][4], yc[QP_NTA];
#pragma unroll
    for (int I = 0; I < QP_NTA; ++I) {
        yc[I] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) yr[I][r] = 0.0;
    }
#pragma unroll
    for (int I = 0; I < QP_NTA; ++I) {
        double wr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) wr[r] = w[16 * I + rg + 4 * r];
#pragma unroll
        for (int J = 0; J <= I; ++J) {
            const double wj = w[16 * J + cl];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double hv = Ht[TI(I, J)][r];
                yr[I][r] = fma(hv, wj, yr[I][r]);
                if (I != J) yc[J] = fma(hv, wr[r], yc[J]);
            }
        }
    }
    const bool hi8 = (cl & 8) != 0, hi4 = (cl & 4) != 0;
#pragma unroll
    for (int I = 0; I < QP_NTA; ++I) {
        row_sum16x4(yr[I], hi8, hi4);
        yc[I] = col_sum4(yc[I]);
    }
    if (cl == 0) {
#pragma unroll
        for (int I = 0; I < QP_NTA; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[16 * I + rg + 4 * r] = yr[I][r];
    }
    wave_sync();
    if (rg == 0) {
#pragma unroll
        for (int I = 0; I < QP_NTA; ++I) out[16 * I + cl] += yc[I];
    }
    wave_sync();
}

// Two-phase solve of the fast instance (MODE of qp_tiled_body<false, MODE>):
//   QP_WHOLE   the solve in one launch
//   QP_FIRST   the same up to the top of iteration QP_SPLIT_IT: a kite that
//              passes the freeze test there (or earlier) finishes as in the
//              whole solve; any other stores the state the loop carries across
//              an iteration (checkpoint, below) and a dispatch key taken from
//              its residual, and ends
//   QP_RESUME  the constants of the solve as in the whole instance, the
//              iterate from the checkpoint, the loop from it = QP_SPLIT_IT
// The resumed kites are dispatched by their residual at the split, largest
// first: a key from inside the solve predicts the remaining iterations, which
// the previous step's count (k_qp_order on iters) barely does (DESIGN 4.3).
// No operation changes or moves, so the result is bitwise the whole solve's.
//
// Checkpoint of kite b: QP_CK_SLOTS x 64 doubles at ckpt + b * QP_CK_DOUBLES,
// slot-major (one coalesced store / load per slot):
//   0..15  w, sl, su, zl, zu, rd, rpl, rpu (two slots each)
//   16..21 slo, shi, zlo, zhi, rplo, rphi
//   22     lane 0: mu, lane 1: rmax_prev, lane 2: resid (after residuals())
// q.cw and a_prev are rewritten before they are read again.
// Key of kite b: 0 when the first phase finished it, else 1 + the binary
// exponent of resid clamped into [QP_KEY_EMIN, QP_KEY_EMIN + QP_KEY_BINS - 2].
constexpr int QP_WHOLE = 0, QP_FIRST = 1, QP_RESUME = 2;
#ifndef QP_SPLIT_IT
#define QP_SPLIT_IT 9
#endif
constexpr int QP_CK_SLOTS = 23;
constexpr int QP_CK_DOUBLES = QP_CK_SLOTS * 64;
constexpr int QP_KEY_BINS = 64;        // keys 0 .. 63
constexpr int QP_KEY_EMIN = -40;       // 2^-40 ~ 9e-13 < IPM_FREEZE: no live kite lies below

template <bool LAZY, int MODE = QP_WHOLE>
__device__ __forceinline__ void qp_tiled_body(int b, ModelConst /*P*/, RtiConst C, int B,
                                                    const double* __restrict__ Htl,
                                                    const double* __restrict__ Habp,
                                                    const double* __restrict__ Hbbp,
                                                    const double* __restrict__ hs, const double* __restrict__ Cr,
                                                    const double* __restrict__ clp, const double* __restrict__ cup,
                                                    const double* __restrict__ hmaxp,
                                                    const double* __restrict__ AB, const double* __restrict__ DEF,
                                                    double* __restrict__ X, double* __restrict__ U,
                                                    double* __restrict__ u0_out, double* __restrict__ diag,
                                                    int32_t* __restrict__ status, double* __restrict__ kkt_out,
                                                    int32_t* __restrict__ iters_out, int32_t* __restrict__ lazy, double* __restrict__ wstep,
                                                    double* __restrict__ ckpt = nullptr,
                                                    int32_t* __restrict__ key = nullptr) {
    static_assert(!LAZY || MODE == QP_WHOLE, "the lazy instance is not split");
    if constexpr (MODE == QP_RESUME) {
        if (key[b] == 0) return;                       // finished by the first phase
    }
    __shared__ double sT[QP_NTA * 16 * TLD];
    __shared__ double sP[(QP_NTA - 1) * 16 * TLD];
    __shared__ double sC[(QN + LAZY_ROWS) * QNC];   // vx-bound rows (kite controls only), then lazy rows
    __shared__ double sHab[2 * QNA];
    __shared__ double sV0[QNA], sV1[QNA];
    __shared__ double sQ[QN + LAZY_ROWS];
    __shared__ double sD[QNA];
    __shared__ double sE[QNA];          // equilibration E of the current factorization
    __shared__ double sY[2 * QNA];      // Y = L^-1 E M_ab (col layout source)
    __shared__ double sLb[4 * QN + 2], sUb[4 * QN + 2], sHv[4 * QN + 2];
    __shared__ double vec[QNA + 8];
    __shared__ double sbnd[32], sXc[LAZY_ROWS];
    __shared__ int sel[3 * LAZY_ROWS];

    const int l = threadIdx.x;
    const int N = C.N, n = C.n;            // n = 82, N = 20
#ifdef KITE_QP_PROF
    unsigned long long prof_acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long prof_sub[3] = {0, 0, 0};
    unsigned long long prof_wsub[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long prof_last = __builtin_amdgcn_s_memtime();
    unsigned long long prof_wt = prof_last;
#endif
    double* Xb = X + (size_t)b * (N + 1) * NX;
    double* Ub = U + (size_t)b * N * NU;

    // ---- load the QP (H_aa tiles stay in global / L2: re-read per iteration) --
    const double* Hg = Htl + (size_t)b * QP_NTILE * 256;
    double4v Mt[QP_NTILE];
    // Every global load of the kite is issued here, before the first wait, in
    // the order of use (the waits then drain in that order: the small vectors
    // first, the 30 loads of H last), so a kite starts with one exposed round
    // trip instead of one per group.  Compile-time trip counts (N == QN,
    // n == 4 QN + 2 on this path); lanes past an array's end load a clamped
    // element and drop it, so no load sits behind a branch.
    // H_aa tiles -> Mt (lane order [tile][reg pair][lane][2]: a lane's registers
    // r, r + 1 are adjacent, so a tile is two 16-byte loads per lane); they
    // serve the residual mat-vec and then become the normal matrix
    auto load_h = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < QP_NTILE; ++t)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const double2v v = *reinterpret_cast<const double2v*>(Hg + t * 256 + p * 128 + 2 * l);
                Mt[t][2 * p] = v[0];
                Mt[t][2 * p + 1] = v[1];
            }
    };
    double cv[QN], habv[3], ubv[2], hsv[2], suv[2], lbuv[2], ubuv[2];
#pragma unroll
    for (int k = 0; k < QN; ++k) cv[k] = Cr[((size_t)b * QN + k) * (4 * QN + 2) + l];   // QNC == 64 == lanes
#pragma unroll
    for (int q2 = 0; q2 < 3; ++q2) {
        const int e = l + 64 * q2 < 2 * QNA ? l + 64 * q2 : 0;
        habv[q2] = Habp[((size_t)b * QNA + e % QNA) * 2 + e / QNA];
    }
    const double hbb00 = Hbbp[(size_t)b * 4 + 0], hbb01 = Hbbp[(size_t)b * 4 + 1], hbb11 = Hbbp[(size_t)b * 4 + 3];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = l + 64 * s;
        // the control that bounds variable i (none for theta0 / thetadot0)
        const int ue = i < 3 * N ? (i / 3) * NU + i % 3 : (i < 4 * N ? (i - 3 * N) * NU + 3 : 0);
        ubv[s] = Ub[ue];
        // its scale and bounds: lane-indexed, so loads like the rest (left in the
        // slot loop below they would each wait for everything issued here)
        const int c = i < 3 * N ? i % 3 : 3;
        suv[s] = C.Su[c]; lbuv[s] = C.lbu[c]; ubuv[s] = C.ubu[c];
        hsv[s] = hs[(size_t)b * n + (i < n ? i : 0)];
    }
    const double clv = clp[(size_t)b * N + (l < N ? l : 0)], cuv = cup[(size_t)b * N + (l < N ? l : 0)];
    const double hmaxv = hmaxp[b];
    // state-bound table sbnd[i] = lbx[i], sbnd[16 + i] = ubx[i]: read by
    // next_round only, so the fast instance has none
    double lbv = 0.0, ubxv = 0.0;
    if constexpr (LAZY) { lbv = C.lbx[l < NX ? l : 0]; ubxv = C.ubx[l < NX ? l : 0]; }
    // resume: the checkpoint, ahead of H (it is used first)
    [[maybe_unused]] double ck[QP_CK_SLOTS];
    if constexpr (MODE == QP_RESUME) {
        const double* cp = ckpt + (size_t)b * QP_CK_DOUBLES + l;
#pragma unroll
        for (int v = 0; v < QP_CK_SLOTS; ++v) ck[v] = cp[v * 64];
    }
    load_h();
    QP_WSUB(0);                                        // init: every load issued
#pragma unroll
    for (int k = 0; k < QN; ++k) sC[k * QNC + l] = cv[k];
#pragma unroll
    for (int q2 = 0; q2 < 3; ++q2)
        if (l + 64 * q2 < 2 * QNA) sHab[l + 64 * q2] = habv[q2];
    if constexpr (LAZY) {
        if (l < NX) { sbnd[l] = lbv; sbnd[16 + l] = ubxv; }
    }

    QPState<2> q;
    const bool has_lo = C.lo_fin != 0, has_hi = C.hi_fin != 0;
    int m = QN;                                        // rows in use: N vx rows + lazy rows
    int nI = 2 * n + N * ((has_lo ? 1 : 0) + (has_hi ? 1 : 0));
    bool row_lane = l < N;
    // finite sides of a row lane: the lazy rows (lanes >= QN) are lower bounds;
    // written so that the LAZY = false instance compiles to the plain has_lo / has_hi
#define TQ_LO (has_lo || (LAZY && l >= QN))
#define TQ_HI (has_hi && (!LAZY || l < QN))
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = l + 64 * s;
        double lo = 0.0, hi = 0.0, hv = 0.0;
        if (i < n) {
            if (i < 4 * N) {
                lo = suv[s] * (lbuv[s] - ubv[s]);
                hi = suv[s] * (ubuv[s] - ubv[s]);
            } else if (i == 4 * N) {
                lo = -C.flex * C.Sx13; hi = C.flex * C.Sx13;
            } else {
                lo = -C.flex * C.Sx14; hi = C.flex * C.Sx14;
            }
            hv = hsv[s];
        }
        if (i < n) { sLb[i] = lo; sUb[i] = hi; sHv[i] = hv; }     // constants of the solve: LDS
        const double mar = 0.1 * (hi - lo);
        double w0 = 0.0;
        if (w0 < lo + mar) w0 = lo + mar;
        if (w0 > hi - mar) w0 = hi - mar;
        q.w[s] = (i < n) ? w0 : 0.0;
        q.sl[s] = fmax(q.w[s] - lo, IPM_S0);
        q.su[s] = fmax(hi - q.w[s], IPM_S0);
        q.zl[s] = IPM_Z0; q.zu[s] = IPM_Z0;
    }
    q.clo = row_lane ? clv : 0.0;
    q.chi = row_lane ? cuv : 0.0;
    const double dscale = 1.0 / (1.0 + hmaxv);
    double inI = 1.0 / (double)nI;
    wave_sync();

    // ---- helpers -------------------------------------------------------------
    auto put_a = [&](double* dst, const double v[2]) __attribute__((always_inline)) {      // slots -> LDS (first 80 entries)
        dst[l] = v[0];
        if (l < QNA - 64) dst[64 + l] = v[1];
    };
    auto get_b = [&](const double v[2], double& b0, double& b1) __attribute__((always_inline)) {
        b0 = readlane_d(v[1], QNA - 64);
        b1 = readlane_d(v[1], QNA - 64 + 1);
    };
    // C x on row lanes (x in LDS): row k's 64-long dot product is split over
    // lanes k, k + 20, k + 40 (22 / 22 / 20 columns) and summed by bpermute
    auto rows_times = [&](const double* x) __attribute__((always_inline)) -> double {
        double t = 0.0;
        if (l < 3 * QN) {
            // 22 / 22 / 20 columns per lane, two independent partial sums
            const int k = l % QN, p = l / QN;
            const double* cr = sC + k * QNC + 22 * p;
            const double* xp = x + 22 * p;
            const bool full = p < 2;
            double t0 = 0.0, t1 = 0.0;
#pragma unroll
            for (int j = 0; j < 20; j += 2) {
                t0 = fma(cr[j], xp[j], t0);
                t1 = fma(cr[j + 1], xp[j + 1], t1);
            }
            if (full) { t0 = fma(cr[20], xp[20], t0); t1 = fma(cr[21], xp[21], t1); }
            t = t0 + t1;
        }
        t += __shfl(t, l + QN, 64) + __shfl(t, l + 2 * QN, 64);
        double te = 0.0;
        if (m > QN) {                                  // lazy rows: lanes 60.. compute, lanes QN.. own them
            if (l >= 3 * QN && l - 3 * QN < m - QN) {
                const double* cr = sC + (l - 2 * QN) * QNC;
                for (int j = 0; j < 3 * QN; ++j) te = fma(cr[j], x[j], te);
            }
            te = __shfl(te, l + 2 * QN, 64);
        }
        if constexpr (LAZY) return l < QN ? t : (row_lane ? te : 0.0);
        return row_lane ? t : 0.0;
    };
    auto rows_T = [&](const double* y, double out[2]) {    // C' y (y in LDS, N)
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;    // slot 0 = columns 0..63, slot 1 has no C entries
#pragma unroll
        for (int k = 0; k < QN; k += 4) {                  // N == QN on this path
            t0 = fma(sC[k * QNC + l], y[k], t0);
            t1 = fma(sC[(k + 1) * QNC + l], y[k + 1], t1);
            t2 = fma(sC[(k + 2) * QNC + l], y[k + 2], t2);
            t3 = fma(sC[(k + 3) * QNC + l], y[k + 3], t3);
        }
        for (int k = QN; k < m; ++k) t0 = fma(sC[k * QNC + l], y[k], t0);
        out[0] = (t0 + t1) + (t2 + t3);
        out[1] = 0.0;
    };

    double resid = 0.0;
    // Recursive residuals (oracle qp_ipm, cfg C_qp_rec = QP_REC_THR): with one
    // step length a for w, s, z the linear residuals shrink exactly by (1 - a);
    // while max((1 - a) rmax, mu) >= QP_REC_THR (mu above the stall floor) an
    // iteration scales the previous residual vectors instead of forming H w,
    // C w and C' z -- below it, and so for every freeze decision, exactly.
    // First solve only: the re-solves with lazy rows evaluate them every time.
    double a_prev = 0.0, rmax_prev = INFINITY;
    auto residuals = [&](bool may_rec) __attribute__((always_inline)) -> double {
        // mu first (the same terms in the same order as the exact pass summed them)
        double mu = 0.0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = l + 64 * s;
            if (i < n) mu += q.sl[s] * q.zl[s] + q.su[s] * q.zu[s];
        }
        if (row_lane) {
            if (TQ_LO) mu += q.slo * q.zlo;
            if (TQ_HI) mu += q.shi * q.zhi;
        }
        mu = uniform_d(wave_sum(mu) * inI);
        if (may_rec && mu >= IPM_MU_FLOOR && nmax((1.0 - a_prev) * rmax_prev, mu) >= QP_REC_THR) {
            const double f = 1.0 - a_prev;
            double rmax = 0.0;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                q.rd[s] *= f; q.rpl[s] *= f; q.rpu[s] *= f;     // zero past n
                rmax = nmax(rmax, fabs(q.rd[s]) * dscale);
                rmax = nmax(rmax, fmax(fabs(q.rpl[s]), fabs(q.rpu[s])));
            }
            q.rplo *= f; q.rphi *= f;                           // zero off the row lanes
            rmax = nmax(rmax, fmax(fabs(q.rplo), fabs(q.rphi)));
            rmax_prev = uniform_d(wave_nmax(rmax));
            resid = uniform_d(nmax(rmax_prev, mu));
            return mu;
        }
        put_a(sV0, q.w);
        double wb0, wb1;
        get_b(q.w, wb0, wb1);
        wave_sync();
        // Mt = H_aa (load_h: before the loop, then issued by the corrector as
        // soon as its solve is done, so the loads fly under the step update)
        tile_symv(Mt, sV0, sV1, l);
        q.cw = rows_times(sV0);
        // H_ba w_a
        double hb0 = 0.0, hb1 = 0.0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = l + 64 * s;
            if (i < QNA) { hb0 = fma(sHab[i], q.w[s], hb0); hb1 = fma(sHab[QNA + i], q.w[s], hb1); }
        }
        hb0 = uniform_d(wave_sum(hb0)); hb1 = uniform_d(wave_sum(hb1));
        wave_sync();
        if (row_lane) vec[l] = (TQ_LO ? q.zlo : 0.0) - (TQ_HI ? q.zhi : 0.0);
        wave_sync();
        double ctz[2];
        rows_T(vec, ctz);
        double rmax = 0.0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = l + 64 * s;
            if (i < n) {
                double hw;
                if (i < QNA) hw = sV1[i] + sHab[i] * wb0 + sHab[QNA + i] * wb1;
                else if (i == QNA) hw = hb0 + hbb00 * wb0 + hbb01 * wb1;
                else hw = hb1 + hbb01 * wb0 + hbb11 * wb1;
                q.rd[s] = hw + sHv[i] - (q.zl[s] - q.zu[s]) - ctz[s];
                q.rpl[s] = q.w[s] - sLb[i] - q.sl[s];
                q.rpu[s] = sUb[i] - q.w[s] - q.su[s];
                rmax = nmax(rmax, fabs(q.rd[s]) * dscale);
                rmax = nmax(rmax, fmax(fabs(q.rpl[s]), fabs(q.rpu[s])));
            } else {
                q.rd[s] = 0.0; q.rpl[s] = 0.0; q.rpu[s] = 0.0;
            }
        }
        q.rplo = 0.0; q.rphi = 0.0;
        if (row_lane) {
            if (TQ_LO) { q.rplo = q.cw - q.clo - q.slo; rmax = nmax(rmax, fabs(q.rplo)); }
            if (TQ_HI) { q.rphi = q.chi - q.cw - q.shi; rmax = nmax(rmax, fabs(q.rphi)); }
        }
        rmax_prev = uniform_d(wave_nmax(rmax));
        resid = uniform_d(nmax(rmax_prev, mu));
        wave_sync();
        return mu;
    };

    // initial slacks of the general rows
    auto init_rows = [&]() __attribute__((always_inline)) {
        put_a(sV0, q.w);
        wave_sync();
        q.cw = rows_times(sV0);
        q.slo = row_lane && TQ_LO ? fmax(q.cw - q.clo, IPM_S0) : 1.0;
        q.shi = row_lane && TQ_HI ? fmax(q.chi - q.cw, IPM_S0) : 1.0;
        q.zlo = row_lane && TQ_LO ? IPM_Z0 : 0.0;
        q.zhi = row_lane && TQ_HI ? IPM_Z0 : 0.0;
        wave_sync();
    };
    [[maybe_unused]] double mu_ck = 0.0;
    if constexpr (MODE == QP_RESUME) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            q.w[s] = ck[s]; q.sl[s] = ck[2 + s]; q.su[s] = ck[4 + s]; q.zl[s] = ck[6 + s]; q.zu[s] = ck[8 + s];
            q.rd[s] = ck[10 + s]; q.rpl[s] = ck[12 + s]; q.rpu[s] = ck[14 + s];
        }
        q.slo = ck[16]; q.shi = ck[17]; q.zlo = ck[18]; q.zhi = ck[19]; q.rplo = ck[20]; q.rphi = ck[21];
        q.cw = 0.0;                                    // rewritten by the next exact residuals before any use
        mu_ck = uniform_d(readlane_d(ck[22], 0));
        rmax_prev = uniform_d(readlane_d(ck[22], 1));
        resid = uniform_d(readlane_d(ck[22], 2));
    } else {
        init_rows();
    }
    QP_WSUB(1);                                        // init: small vectors consumed (first waits done)
    QP_WDRAIN(2);                                      // init: H arrived

    double sgl[2], sgu[2], sglo = 0.0, sghi = 0.0;
    double isl[2], isu[2], islo = 1.0, ishi = 1.0;     // reciprocal slacks of the current iterate
    double ls00 = 1.0, ls10 = 0.0, ls11 = 1.0;        // Cholesky of the theta Schur complement
    double il00 = 1.0, il11 = 1.0;                    // and its reciprocal diagonal

    const int cl = l & 15, rg = l >> 4;
    const bool hi8 = (cl & 8) != 0, hi4 = (cl & 4) != 0;
    const double* tl = sT + cl * TLD + rg;

    // x <- M^-1 x  (x in slots)
    auto msolve = [&](double x[2]) __attribute__((always_inline)) {
        double rb0, rb1;
        get_b(x, rb0, rb1);
        put_a(sV0, x);
        wave_sync();
        double rr[QP_NTA][4], ua[QP_NTA];
        fwd_solve(Mt, tl, sV0, sE, rg, hi8, hi4, ua);            // u_a = L^-1 E r_a
        // u_b = Ls^-1 (r_b - Y' u_a)
        double t0 = 0.0, t1 = 0.0;
#pragma unroll
        for (int K = 0; K < QP_NTA; ++K) {
            t0 = fma(sY[16 * K + cl], ua[K], t0);
            t1 = fma(sY[QNA + 16 * K + cl], ua[K], t1);
        }
        t0 = uniform_d(row_sum16(t0)); t1 = uniform_d(row_sum16(t1));   // col layout: the same in every row
        const double ub0 = (rb0 - t0) * il00;
        const double ub1 = (rb1 - t1 - ls10 * ub0) * il11;
        const double xb1 = ub1 * il11;
        const double xb0 = (ub0 - ls10 * xb1) * il00;
#pragma unroll
        for (int K = 0; K < QP_NTA; ++K) ua[K] = ua[K] - sY[16 * K + cl] * xb0 - sY[QNA + 16 * K + cl] * xb1;
        bwd_solve(Mt, tl, ua, hi8, hi4, rr);                     // x_a = E L^-T (u_a - Y x_b), row layout
        wave_sync();
        if (cl == 0) {
#pragma unroll
            for (int K = 0; K < QP_NTA; ++K)
#pragma unroll
                for (int r = 0; r < 4; ++r) sV0[16 * K + rg + 4 * r] = rr[K][r] * sE[16 * K + rg + 4 * r];
        }
        wave_sync();
        x[0] = sV0[l];
        x[1] = (l < QNA - 64) ? sV0[64 + l] : (l == QNA - 64 ? xb0 : (l == QNA - 64 + 1 ? xb1 : 0.0));
        wave_sync();
    };

    struct Dir { double dw[2], dsl[2], dsu[2], dzl[2], dzu[2], dslo, dshi, dzlo, dzhi; };
    auto newton = [&](const double rcl[2], const double rcu[2], double rclo, double rchi, Dir& D,
                      bool reload_h) __attribute__((always_inline)) {
        double t_lo = 0.0, t_hi = 0.0;
        if (row_lane) {
            if (TQ_LO) t_lo = rclo * islo - sglo * q.rplo;
            if (TQ_HI) t_hi = rchi * ishi - sghi * q.rphi;
        }
        wave_sync();
        if (row_lane) vec[l] = t_lo - t_hi;
        wave_sync();
        double ct[2];
        rows_T(vec, ct);
        double r[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = l + 64 * s;
            if (i < n) {
                const double tl = rcl[s] * isl[s] - sgl[s] * q.rpl[s];
                const double tu = rcu[s] * isu[s] - sgu[s] * q.rpu[s];
                r[s] = -q.rd[s] + (tl - tu) + ct[s];
            } else {
                r[s] = 0.0;
            }
        }
        wave_sync();
        msolve(r);
        if (reload_h) load_h();                        // the factor is dead after the corrector's solve
        put_a(sV1, r);
        wave_sync();
        const double cdw = rows_times(sV1);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            D.dw[s] = r[s];
            D.dsl[s] = r[s] + q.rpl[s];
            D.dsu[s] = -r[s] + q.rpu[s];
            D.dzl[s] = (rcl[s] - q.zl[s] * D.dsl[s]) * isl[s];
            D.dzu[s] = (rcu[s] - q.zu[s] * D.dsu[s]) * isu[s];
        }
        D.dslo = 0.0; D.dshi = 0.0; D.dzlo = 0.0; D.dzhi = 0.0;
        if (row_lane) {
            if (TQ_LO) { D.dslo = cdw + q.rplo; D.dzlo = (rclo - q.zlo * D.dslo) * islo; }
            if (TQ_HI) { D.dshi = -cdw + q.rphi; D.dzhi = (rchi - q.zhi * D.dshi) * ishi; }
        }
        wave_sync();
    };
    // step length to the boundary: min over the rows with a negative step of
    // -v / dv = 1 / max(1, max(-dv / v)); -dv / v as -dv * (1/v), the slacks'
    // reciprocals of this iterate (isl, isu, islo, ishi) and the multipliers'
    // computed here -- a multiply and a max per row, no branch, one reciprocal
    // per wave (rows with dv >= 0 give -dv / v <= 0 and never raise the max;
    // a NaN direction is dropped by v_max_f64, as by the compare before)
    auto max_step = [&](const Dir& D) __attribute__((always_inline)) -> double {
        double m = 1.0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            m = fmax(m, -D.dsl[s] * isl[s]);
            m = fmax(m, -D.dsu[s] * isu[s]);
            m = fmax(m, -D.dzl[s] * fast_rcp(q.zl[s]));
            m = fmax(m, -D.dzu[s] * fast_rcp(q.zu[s]));
        }
        if (TQ_LO) {                                   // off the row lanes dslo = dzlo = 0
            m = fmax(m, -D.dslo * islo);
            m = fmax(m, -D.dzlo * fast_rcp(row_lane ? q.zlo : 1.0));
        }
        if (TQ_HI) {
            m = fmax(m, -D.dshi * ishi);
            m = fmax(m, -D.dzhi * fast_rcp(row_lane ? q.zhi : 1.0));
        }
        return rcp_d(wave_max(m));
    };

    int iters = C.K;
    double kkt = 0.0;
    double* dxs = sP;                                  // Cholesky panels are dead after the last solve
    double* viol = sP + (QN + 1) * 16;
    QP_MARK(0);
    // bound check of round `round` on the accepted iterate and, for a kite still
    // outside its state box, the next rows and a cold restart (false: commit)
    int added = 0;
    auto next_round = [&](int round) __attribute__((always_inline)) -> bool {
        const bool outside = rti_expand<2, true>(C, b, l, q.w, kkt < QP_STEP_ACCEPT, AB, DEF, Xb, sbnd, vec, dxs);
        if (!outside || !(kkt < QP_STEP_ACCEPT) || round == LAZY_ROUNDS || added == LAZY_ROWS) return false;
        const int cnt = lazy_select<true>(C, l, Xb, dxs, sbnd, viol, sel, LAZY_ROWS - added);
        if (cnt == 0) return false;
        // violated state bounds: rows appended, the QP solved again from a cold start
        put_a(sV0, q.w);                                   // scaled w (the lazy rows use columns < 60)
        wave_sync();
        for (int t = 0; t < cnt; ++t) {
            const double cv = lazy_row<true>(C, b, l, sel[3 * t], sel[3 * t + 1], sel[3 * t + 2], AB, Xb, dxs, sbnd,
                                             sV0, sC + (size_t)m * QNC, QNC);
            if (l == 0) sXc[m - QN] = cv;
            ++m;
            wave_sync();
        }
        added += cnt;
        nI += cnt;
        inI = 1.0 / (double)nI;
        row_lane = l < m;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = l + 64 * s;
            const double lo = i < n ? sLb[i] : 0.0, hi = i < n ? sUb[i] : 0.0;
            const double mar = 0.1 * (hi - lo);
            double w0 = 0.0;
            if (w0 < lo + mar) w0 = lo + mar;
            if (w0 > hi - mar) w0 = hi - mar;
            q.w[s] = (i < n) ? w0 : 0.0;
            q.sl[s] = fmax(q.w[s] - lo, IPM_S0);
            q.su[s] = fmax(hi - q.w[s], IPM_S0);
            q.zl[s] = IPM_Z0; q.zu[s] = IPM_Z0;
        }
        if (l >= QN) { q.clo = row_lane ? sXc[l - QN] : 0.0; q.chi = 0.0; }
        init_rows();
        load_h();
        return true;
    };
    bool more = true;
    if constexpr (LAZY) {
        // the fast instance solved round 0 and k_expand20 listed this kite: its
        // scaled solution, residual and iteration count are handed over (wstep
        // + B n, kkt_out, iters_out), so the lazy instance starts at round 0's
        // bound check instead of solving round 0 again -- bitwise the same
        // iterate, one serial QP solve less per listed kite
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = l + 64 * s;
            q.w[s] = i < n ? wstep[(size_t)B * n + (size_t)b * n + i] : 0.0;
        }
        kkt = kkt_out[b];
        iters = iters_out[b];
        more = next_round(0);
    }
    for (int round = LAZY ? 1 : 0; more; ++round) {
    iters = C.K;
    [[maybe_unused]] const int kfirst = C.K > QP_SPLIT_IT ? QP_SPLIT_IT : C.K;   // the first phase's cap
    for (int it = MODE == QP_RESUME ? QP_SPLIT_IT : 0; MODE == QP_FIRST ? it < kfirst : it < C.K; ++it) {
        // the lazy instance only re-solves with state-bound rows: exact residuals
        // there.  Such a re-solve starts far outside its new rows and can run into
        // the cap K; under the recursion the capped iterate then follows rounding
        // (the oracle's own plan moved by up to 3e-3 under a 1e-15 relative change
        // of its inputs, 1.7e-6 with exact residuals; tests/test_envelope.py)
        double mu_;
        if constexpr (MODE == QP_RESUME) {             // the split iteration's residuals come from the checkpoint
            if (it == QP_SPLIT_IT) mu_ = mu_ck; else mu_ = residuals(true);
        } else {
            mu_ = residuals(!LAZY && it > 0);
        }
        const double mu = mu_;
        QP_MARK(1);
        QP_WSTART();
        if (resid < IPM_FREEZE || resid != resid || mu < IPM_MU_FLOOR) { iters = it; break; }   // converged, poisoned or stalled
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            isl[s] = fast_rcp(q.sl[s]);
            isu[s] = fast_rcp(q.su[s]);
            sgl[s] = q.zl[s] * isl[s];
            sgu[s] = q.zu[s] * isu[s];
        }
        islo = fast_rcp(q.slo);                       // slo = shi = 1 off the row lanes
        ishi = fast_rcp(q.shi);
        sglo = (row_lane && TQ_LO) ? q.zlo * islo : 0.0;
        sghi = (row_lane && TQ_HI) ? q.zhi * ishi : 0.0;
        // ---- normal matrix: tiles = H_aa + diag + C' Sigma_c C -------------
        if (row_lane) sQ[l] = sqrt(sglo + sghi);
        {
            double dsum[2] = {sgl[0] + sgu[0], sgl[1] + sgu[1]};
            put_a(sD, dsum);
        }
        double sb0, sb1;
        {
            const double d1 = sgl[1] + sgu[1];
            sb0 = readlane_d(d1, QNA - 64);
            sb1 = readlane_d(d1, QNA - 64 + 1);
        }
        wave_sync();
        QP_WSUB(3);                                    // normal matrix: up to the first MFMA's wait
        QP_WDRAIN(4);                                  // normal matrix: the reloaded H arrived
        {                                              // Mt = H_aa (loaded by residuals())
            // vx row k depends on the kite controls of intervals 0..k only
            // (columns < 3k + 3; the condensing leaves exact zeros past them):
            // the k-step of rows 4ks..4ks+3 touches tile columns 0..(12ks+11)/16
            // -- 26 MFMAs instead of 50, the same sums (the skipped products are
            // exact zeros)
#pragma unroll
            for (int ks = 0; ks < QN / 4; ++ks) {
                const int kr = 4 * ks + rg;
                const int imax = (12 * ks + 11) / 16;
                const double sc = sQ[kr];
                double fr[4];
#pragma unroll
                for (int I = 0; I < 4; ++I) fr[I] = I <= imax ? sC[kr * QNC + 16 * I + cl] * sc : 0.0;
#pragma unroll
                for (int I = 0; I < 4; ++I)
#pragma unroll
                    for (int J = 0; J <= I; ++J)
                        if (I <= imax)
                            Mt[TI(I, J)] = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[I], fr[J], Mt[TI(I, J)], 0, 0, 0);
            }
            if (m > QN) {                              // lazy rows: one more k-step (rows QN .. QN + 3)
                const int kr = QN + rg;
                const double sc = kr < m ? sQ[kr] : 0.0;
                double fr[4];
#pragma unroll
                for (int I = 0; I < 4; ++I) fr[I] = kr < m ? sC[kr * QNC + 16 * I + cl] * sc : 0.0;
#pragma unroll
                for (int I = 0; I < 4; ++I)
#pragma unroll
                    for (int J = 0; J <= I; ++J)
                        Mt[TI(I, J)] = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[I], fr[J], Mt[TI(I, J)], 0, 0, 0);
            }
#pragma unroll
            for (int K = 0; K < QP_NTA; ++K) {
                const double dk = sD[16 * K + cl];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (rg + 4 * r == cl) Mt[TI(K, K)][r] += dk;
            }
            // equilibrate M_aa <- E M_aa E, E = diag(M_aa)^-1/2: the barrier
            // weights spread the diagonal over ~24 decades near convergence,
            // and the diagonal tiles are inverted explicitly below
#pragma unroll
            for (int K = 0; K < QP_NTA; ++K) {
                const double4v& mk = Mt[TI(K, K)];           // diagonal: register cl >> 2 of row-group cl & 3
                const int rd = cl >> 2;
                const double d = rd == 0 ? mk[0] : rd == 1 ? mk[1] : rd == 2 ? mk[2] : mk[3];
                if ((cl & 3) == rg) sE[16 * K + cl] = fast_rsq(piv_fix(d));
            }
            wave_sync();
#pragma unroll
            for (int I = 0; I < QP_NTA; ++I)
#pragma unroll
                for (int J = 0; J <= I; ++J) {
                    const double ec = sE[16 * J + cl];
#pragma unroll
                    for (int r = 0; r < 4; ++r) Mt[TI(I, J)][r] *= sE[16 * I + rg + 4 * r] * ec;
                    asm volatile("s_nop 0" ::: "memory");   // keep the E loads next to their use
                }
        }
        wave_sync();
        QP_WSUB(5);                                    // normal matrix: MFMAs, diagonal, equilibration
        QP_MARK(2);
#ifdef KITE_QP_PROF
        chol_tiles(Mt, sT, sP, l, prof_sub);
#else
        chol_tiles(Mt, sT, sP, l);
#endif
        QP_MARK(3);
        // ---- theta Schur complement -----------------------------------------
        {
            double Y0[QP_NTA], Y1[QP_NTA];             // col layout
            fwd_solve2(Mt, tl, sHab, sHab + QNA, sE, rg, hi8, hi4, Y0, Y1);   // Y = L^-1 E M_ab  (E M_aa E = L L')
            double y00 = 0.0, y01 = 0.0, y11 = 0.0;
#pragma unroll
            for (int K = 0; K < QP_NTA; ++K) {
                y00 = fma(Y0[K], Y0[K], y00); y01 = fma(Y0[K], Y1[K], y01); y11 = fma(Y1[K], Y1[K], y11);
                if (rg == 0) { sY[16 * K + cl] = Y0[K]; sY[QNA + 16 * K + cl] = Y1[K]; }
            }
            y00 = row_sum16(y00); y01 = row_sum16(y01); y11 = row_sum16(y11);
            const double s00 = hbb00 + sb0 - y00, s01 = hbb01 - y01, s11 = hbb11 + sb1 - y11;
            ls00 = sqrt(piv_fix(s00));
            il00 = fast_rcp(ls00);
            ls10 = s01 * il00;
            ls11 = sqrt(piv_fix(s11 - ls10 * ls10));
            il11 = fast_rcp(ls11);
            // wave-uniform for both solves: keep them in SGPRs
            ls00 = uniform_d(ls00); ls10 = uniform_d(ls10); ls11 = uniform_d(ls11);
            il00 = uniform_d(il00); il11 = uniform_d(il11);
        }
        wave_sync();
        QP_MARK(4);
        // ---- predictor --------------------------------------------------------
        double rcl[2], rcu[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) { rcl[s] = -q.sl[s] * q.zl[s]; rcu[s] = -q.su[s] * q.zu[s]; }
        double rclo = -q.slo * q.zlo, rchi = -q.shi * q.zhi;
        Dir Da;
        newton(rcl, rcu, rclo, rchi, Da, false);
        const double aa = uniform_d(max_step(Da));
        double mua = 0.0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = l + 64 * s;
            if (i < n)
                mua += (q.sl[s] + aa * Da.dsl[s]) * (q.zl[s] + aa * Da.dzl[s]) +
                       (q.su[s] + aa * Da.dsu[s]) * (q.zu[s] + aa * Da.dzu[s]);
        }
        if (row_lane) {
            if (TQ_LO) mua += (q.slo + aa * Da.dslo) * (q.zlo + aa * Da.dzlo);
            if (TQ_HI) mua += (q.shi + aa * Da.dshi) * (q.zhi + aa * Da.dzhi);
        }
        mua = wave_sum(mua) * inI;
        double sigma = uniform_d(mua * fast_rcp(mu));
        sigma = sigma * sigma * sigma;
        QP_MARK(5);
        // ---- corrector --------------------------------------------------------
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            rcl[s] = -q.sl[s] * q.zl[s] - Da.dsl[s] * Da.dzl[s] + sigma * mu;
            rcu[s] = -q.su[s] * q.zu[s] - Da.dsu[s] * Da.dzu[s] + sigma * mu;
        }
        rclo = row_lane && TQ_LO ? -q.slo * q.zlo - Da.dslo * Da.dzlo + sigma * mu : 0.0;
        rchi = row_lane && TQ_HI ? -q.shi * q.zhi - Da.dshi * Da.dzhi + sigma * mu : 0.0;
        Dir Dc;
        newton(rcl, rcu, rclo, rchi, Dc, true);
        const double a = uniform_d(fmin(1.0, fmax(IPM_TAU, 1.0 - mu) * max_step(Dc)));   // tau_k -> 1 (oracle qp_ipm)
        a_prev = a;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            q.w[s] += a * Dc.dw[s];
            q.sl[s] += a * Dc.dsl[s]; q.su[s] += a * Dc.dsu[s];
            q.zl[s] += a * Dc.dzl[s]; q.zu[s] += a * Dc.dzu[s];
        }
        if (row_lane) {
            if (TQ_LO) { q.slo += a * Dc.dslo; q.zlo += a * Dc.dzlo; }
            if (TQ_HI) { q.shi += a * Dc.dshi; q.zhi += a * Dc.dzhi; }
        }
        QP_MARK(6);
    }
    if constexpr (MODE == QP_FIRST) {
        // the top of iteration QP_SPLIT_IT, outside the loop (an exit inside it
        // costs the loop its register allocation): the whole solve's
        // residuals and freeze test, then the hand-over
        static_assert(QP_SPLIT_IT >= 1, "the split iteration may take the recursive residuals");
        if (iters == C.K && C.K > QP_SPLIT_IT) {       // no exit before the split
            const double mu = residuals(true);
            QP_MARK(1);
            if (resid < IPM_FREEZE || resid != resid || mu < IPM_MU_FLOOR) {
                iters = QP_SPLIT_IT;
            } else {
        // (the addresses are formed here: hoisted out of the loop they
        // would stay live through every iteration)
        size_t off = (size_t)b * QP_CK_DOUBLES + l;
        asm volatile("" : "+v"(off));
        double* cp = ckpt + off;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            cp[s * 64] = q.w[s]; cp[(2 + s) * 64] = q.sl[s]; cp[(4 + s) * 64] = q.su[s];
            cp[(6 + s) * 64] = q.zl[s]; cp[(8 + s) * 64] = q.zu[s];
            cp[(10 + s) * 64] = q.rd[s]; cp[(12 + s) * 64] = q.rpl[s]; cp[(14 + s) * 64] = q.rpu[s];
        }
        cp[16 * 64] = q.slo; cp[17 * 64] = q.shi; cp[18 * 64] = q.zlo; cp[19 * 64] = q.zhi;
        cp[20 * 64] = q.rplo; cp[21 * 64] = q.rphi;
        cp[22 * 64] = l == 0 ? mu : (l == 1 ? rmax_prev : resid);
        if (l == 0) {
            int e = (int)((__double_as_longlong(resid) >> 52) & 0x7ff) - 1023;
            e = e < QP_KEY_EMIN ? QP_KEY_EMIN : (e > QP_KEY_EMIN + QP_KEY_BINS - 2 ? QP_KEY_EMIN + QP_KEY_BINS - 2 : e);
            key[b] = e - QP_KEY_EMIN + 1;
        }
        QP_PROF_FLUSH(0);
        return;
            }
        }
    }
    residuals(false);
    kkt = resid;
    QP_MARK(7);
    if constexpr (!LAZY) {
        // the expansion, the bound check and the commit run in k_expand20 (four
        // kites per wave, short and wide): hand over the physical step (zero
        // when the QP failed), the residual and the iteration count
        const bool accept = kkt < QP_STEP_ACCEPT;
        const double iS0 = 1.0 / C.Su[0], iS1 = 1.0 / C.Su[1], iS2 = 1.0 / C.Su[2], iS3 = 1.0 / C.Su[3];
        const double iX13 = 1.0 / C.Sx13, iX14 = 1.0 / C.Sx14;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = l + 64 * s;
            const int c = i % 3;
            const double sc = i < 3 * N ? (c == 0 ? iS0 : (c == 1 ? iS1 : iS2))
                                        : (i < 4 * N ? iS3 : (i == 4 * N ? iX13 : iX14));
            if (i < n) {
                wstep[(size_t)b * n + i] = accept ? q.w[s] * sc : 0.0;
                wstep[(size_t)B * n + (size_t)b * n + i] = q.w[s];      // scaled, for k_qp_tiled_lazy
            }
        }
        if (l == 0) {
            if (kkt_out) kkt_out[b] = kkt;
            if (iters_out) iters_out[b] = iters;
            if constexpr (MODE == QP_FIRST) key[b] = 0;       // finished: nothing to resume
        }
#ifdef KITE_QP_PROF
        QP_MARK(8);
        QP_PROF_FLUSH(1);
#endif
        return;
    }
    more = next_round(round);
    }
    rti_commit<true>(C, b, l, kkt, iters, vec, dxs, sbnd, Xb, Ub, u0_out, diag, status, kkt_out, iters_out,
                     iters_out ? iters_out + B : nullptr, B);
#undef TQ_LO
#undef TQ_HI
#ifdef KITE_QP_PROF
    QP_MARK(8);
    QP_PROF_FLUSH(1);
#endif
}

// the fast instance over the whole grid (LPT order); the lazy instance over
// the kites the fast one listed (lazy[0] = count, lazy[1..]), grid-strided
// (separate names: profilers that truncate template arguments keep them apart)
// k_qp_tiled_whole is the solve in one launch; k_qp_tiled the first phase of
// the split solve (the name the profiling tools key on: it is the kernel of
// the large batches they measure) and k_qp_tiled_resume its second phase over
// the second order.
__global__ __launch_bounds__(64, 1) void k_qp_tiled_whole(ModelConst P, RtiConst C, int B,
                                                    const double* __restrict__ Htl,
                                                    const double* __restrict__ Habp,
                                                    const double* __restrict__ Hbbp,
                                                    const double* __restrict__ hs, const double* __restrict__ Cr,
                                                    const double* __restrict__ clp, const double* __restrict__ cup,
                                                    const double* __restrict__ hmaxp,
                                                    const double* __restrict__ AB, const double* __restrict__ DEF,
                                                    double* __restrict__ X, double* __restrict__ U,
                                                    double* __restrict__ u0_out, double* __restrict__ diag,
                                                    int32_t* __restrict__ status, double* __restrict__ kkt_out,
                                                    int32_t* __restrict__ iters_out,
                                                    const int32_t* __restrict__ order, int32_t* __restrict__ lazy,
                                                    double* __restrict__ wstep) {
        qp_tiled_body<false, QP_WHOLE>(order ? order[blockIdx.x] : blockIdx.x, P, C, B, Htl, Habp, Hbbp, hs, Cr, clp, cup, hmaxp, AB, DEF, X, U, u0_out, diag, status, kkt_out, iters_out, lazy, wstep);
}
__global__ __launch_bounds__(64, 1) void k_qp_tiled(ModelConst P, RtiConst C, int B,
                                                    const double* __restrict__ Htl,
                                                    const double* __restrict__ Habp,
                                                    const double* __restrict__ Hbbp,
                                                    const double* __restrict__ hs, const double* __restrict__ Cr,
                                                    const double* __restrict__ clp, const double* __restrict__ cup,
                                                    const double* __restrict__ hmaxp,
                                                    const double* __restrict__ AB, const double* __restrict__ DEF,
                                                    double* __restrict__ X, double* __restrict__ U,
                                                    double* __restrict__ u0_out, double* __restrict__ diag,
                                                    int32_t* __restrict__ status, double* __restrict__ kkt_out,
                                                    int32_t* __restrict__ iters_out,
                                                    const int32_t* __restrict__ order, int32_t* __restrict__ lazy,
                                                    double* __restrict__ wstep,
                                                    double* __restrict__ ckpt, int32_t* __restrict__ key) {
        qp_tiled_body<false, QP_FIRST>(order ? order[blockIdx.x] : blockIdx.x, P, C, B, Htl, Habp, Hbbp, hs, Cr, clp, cup, hmaxp, AB, DEF, X, U, u0_out, diag, status, kkt_out, iters_out, lazy, wstep, ckpt, key);
}
__global__ __launch_bounds__(64, 1) void k_qp_tiled_resume(ModelConst P, RtiConst C, int B,
                                                    const double* __restrict__ Htl,
                                                    const double* __restrict__ Habp,
                                                    const double* __restrict__ Hbbp,
                                                    const double* __restrict__ hs, const double* __restrict__ Cr,
                                                    const double* __restrict__ clp, const double* __restrict__ cup,
                                                    const double* __restrict__ hmaxp,
                                                    const double* __restrict__ AB, const double* __restrict__ DEF,
                                                    double* __restrict__ X, double* __restrict__ U,
                                                    double* __restrict__ u0_out, double* __restrict__ diag,
                                                    int32_t* __restrict__ status, double* __restrict__ kkt_out,
                                                    int32_t* __restrict__ iters_out,
                                                    const int32_t* __restrict__ order, int32_t* __restrict__ lazy,
                                                    double* __restrict__ wstep,
                                                    double* __restrict__ ckpt, int32_t* __restrict__ key) {
        qp_tiled_body<false, QP_RESUME>(order[blockIdx.x], P, C, B, Htl, Habp, Hbbp, hs, Cr, clp, cup, hmaxp, AB, DEF, X, U, u0_out, diag, status, kkt_out, iters_out, lazy, wstep, ckpt, key);
}
__global__ __launch_bounds__(64, 1) void k_qp_tiled_lazy(ModelConst P, RtiConst C, int B,
                                                    const double* __restrict__ Htl,
                                                    const double* __restrict__ Habp,
                                                    const double* __restrict__ Hbbp,
                                                    const double* __restrict__ hs, const double* __restrict__ Cr,
                                                    const double* __restrict__ clp, const double* __restrict__ cup,
                                                    const double* __restrict__ hmaxp,
                                                    const double* __restrict__ AB, const double* __restrict__ DEF,
                                                    double* __restrict__ X, double* __restrict__ U,
                                                    double* __restrict__ u0_out, double* __restrict__ diag,
                                                    int32_t* __restrict__ status, double* __restrict__ kkt_out,
                                                    int32_t* __restrict__ iters_out,
                                                    const int32_t* __restrict__ order, int32_t* __restrict__ lazy,
                                                    double* __restrict__ wstep) {
        const int cnt = lazy[0];
        for (int j = blockIdx.x; j < cnt; j += gridDim.x) {
            qp_tiled_body<true>(lazy[1 + j], P, C, B, Htl, Habp, Hbbp, hs, Cr, clp, cup, hmaxp, AB, DEF, X, U, u0_out, diag, status, kkt_out, iters_out, lazy, wstep);
            __syncthreads();
        }
}

#ifdef KITE_QP_PROF
// tools only: read and clear the phase profile (24 x uint64)
extern "C" int kite_debug_qp_profile(unsigned long long* out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qp_prof), sizeof(g_qp_prof)) != hipSuccess) return -1;
    const unsigned long long z[24] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_qp_prof), z, sizeof(z)) != hipSuccess) return -1;
    return 0;
}
#endif

// out[j] = v of lane j of this 16-lane row (DPP row_newbcast), j = J .. NK-1
template <int J>
__device__ __forceinline__ void bcast_row13(double v, double* out) {
    out[J] = dpp_d<0x150 + J>(v);
    if constexpr (J + 1 < NK) bcast_row13<J + 1>(v, out);
}

// ---------------------------------------------------------------------------
// k_expand20: the epilogue of the fast k_qp_tiled instance, four kites per
// wave (16-lane rows: lane i of row g = state row i of kite 4 blockIdx + g).
// Same arithmetic as rti_expand + rti_commit (same operation order for the
// trajectory; the cost diagnostic sums over a row instead of a wave): dx_0 = 0,
// dx_{k+1} = A_k dx_k + B_k du_k + d_k with dx_k broadcast inside the row by
// DPP row_newbcast, the theta rows in closed form, the bound check on the fly;
// a kite outside its state bounds goes to the lazy list uncommitted
// (k_qp_tiled_lazy redoes it with rows), every other kite is committed.  The
// 20-step chain runs once per wave here instead of once per kite inside the
// one-wave-per-SIMD QP.
__global__ __launch_bounds__(64) void k_expand20(RtiConst C, int B, const double* __restrict__ wstep,
                                                 const double* __restrict__ AB, const double* __restrict__ DEF,
                                                 double* __restrict__ X, double* __restrict__ U,
                                                 double* __restrict__ u0_out, double* __restrict__ diag,
                                                 int32_t* __restrict__ status, const double* __restrict__ kkt_in,
                                                 const int32_t* __restrict__ iters_in, int32_t* __restrict__ iters_acc,
                                                 int32_t* __restrict__ lazy) {
    constexpr int N = QN, n = 4 * QN + 2;
    __shared__ double sv[4][n + 2];
    __shared__ double sdx[4][(N + 1) * 16];
    __shared__ double sbnd[32];
    const int l = threadIdx.x, g = l >> 4, i = l & 15;
    const int braw = blockIdx.x * 4 + g;
    const bool valid = braw < B;
    const int b = valid ? braw : B - 1;                 // loads stay in range; stores guarded
    double* vec = sv[g];
    double* dxs = sdx[g];
    if (l < 16) { sbnd[l] = C.lbx[l < NX ? l : 0]; sbnd[16 + l] = C.ubx[l < NX ? l : 0]; }
    for (int e = i; e < n; e += 16) vec[e] = wstep[(size_t)b * n + e];
    const double kkt = kkt_in[b];
    const bool accept = kkt < QP_STEP_ACCEPT;
    wave_sync();
    // theta / thetadot rows (exact double integrator), lane = node
    {
        const double dth0 = vec[4 * N], dthd0 = vec[4 * N + 1];
        for (int k = i; k <= N; k += 16) {
            double dth = dth0 + (double)k * C.dt * dthd0, dthd = dthd0;
            for (int m = 0; m < k; ++m) {
                const double du = vec[3 * N + m];
                dth += C.dt * C.dt * ((double)(k - m) - 0.5) * du;
                dthd += C.dt * du;
            }
            dxs[k * 16 + 13] = dth;
            dxs[k * 16 + 14] = dthd;
        }
    }
    // kite states: lane i = row i, PD-deep register ring of [A_k | B_k] row i, d_k[i], x_{k+1}[i]
    bool viol = false;
    {
        constexpr int PD = 4;       // 5 and 10 measured: no change (r05y), the kernel is near its HBM bound
        double dx = 0.0;
        const double* ABb = AB + (size_t)b * N * NK * 16;
        const double* DEFb = DEF + (size_t)b * N * NK;
        const double* Xb = X + (size_t)b * (N + 1) * NX;
        const int lr = i < NK ? i : NK - 1;
        const double blo = sbnd[lr], bhi = sbnd[16 + lr];
        const double tlo = blo - bound_tol(blo), thi = bhi + bound_tol(bhi);
        const bool chk = i >= 1 && i < NK;
        double ar[PD][16], dk[PD], xr[PD];
        auto fetch = [&](int k, double* a, double& d, double& xn) __attribute__((always_inline)) {
            const double* p = ABb + ((size_t)k * NK + lr) * 16;
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = p[j];
            d = DEFb[(size_t)k * NK + lr];
            xn = Xb[(k + 1) * NX + lr];
        };
        auto interval = [&](int k, double* ring, double& dring, double& xring) __attribute__((always_inline)) {
            double a[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = ring[j];
            const double d = dring, xn = xring;
            if (k + PD < N) fetch(k + PD, ring, dring, xring);
            double t0 = fma(a[NK], vec[3 * k], d), t1 = a[NK + 1] * vec[3 * k + 1];
            double t2 = a[NK + 2] * vec[3 * k + 2], t3 = 0.0;
            double bx[NK];
            bcast_row13<0>(dx, bx);
#pragma unroll
            for (int j = 0; j < NK; j += 4) {
                t0 = fma(a[j], bx[j], t0);
                if (j + 1 < NK) t1 = fma(a[j + 1], bx[j + 1], t1);
                if (j + 2 < NK) t2 = fma(a[j + 2], bx[j + 2], t2);
                if (j + 3 < NK) t3 = fma(a[j + 3], bx[j + 3], t3);
            }
            dx = (t0 + t1) + (t2 + t3);
            const double xt = xn + dx;
            if (i < NK) dxs[(k + 1) * 16 + i] = xt;     // the committed state (X += dx)
            viol |= chk && (xt < tlo || xt > thi);
        };
#pragma unroll
        for (int q = 0; q < PD; ++q) fetch(q, ar[q], dk[q], xr[q]);
        static_assert(N % PD == 0, "the register ring cycles in whole rounds");
        for (int k0 = 0; k0 < N; k0 += PD) {
#pragma unroll
            for (int q = 0; q < PD; ++q) interval(k0 + q, ar[q], dk[q], xr[q]);
        }
    }
    wave_sync();
    // a row's kite with violations (and an accepted step) -> lazy list, no commit
    const unsigned long long vm = __builtin_amdgcn_ballot_w64(viol);
    const bool outside = ((vm >> (16 * g)) & 0xFFFFull) != 0;
    if (outside && accept) {
        if (i == 0 && valid) lazy[1 + atomicAdd(lazy, 1)] = b;
        return;
    }
    if (!valid) return;
    // commit (rti_commit, one 16-lane row per kite).  Every read-modify-write
    // loads first, all together, then stores: a load behind a store to the
    // same array would wait out the store's round trip, once per element.
    // The kite-state rows need no load (the chain kept x + dx in dxs).
    double* Xb = X + (size_t)b * (N + 1) * NX;
    double* Ub = U + (size_t)b * N * NU;
    {
        constexpr int TQ = (N + 1 + 15) / 16, UQ = (N * NU + 15) / 16;
        double th[TQ][2], uo[UQ];
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
            const int k = i + 16 * q;
            if (k <= N) { th[q][0] = Xb[k * NX + 13]; th[q][1] = Xb[k * NX + 14]; }
        }
#pragma unroll
        for (int q = 0; q < UQ; ++q) {
            const int e = i + 16 * q;
            if (e < N * NU) uo[q] = Ub[e];
        }
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
            const int k = i + 16 * q;
            if (k <= N) {
                Xb[k * NX + 13] = th[q][0] + dxs[k * 16 + 13];
                Xb[k * NX + 14] = th[q][1] + dxs[k * 16 + 14];
            }
        }
#pragma unroll
        for (int q = 0; q < UQ; ++q) {
            const int e = i + 16 * q;
            if (e < N * NU) {
                const int k = e / NU, c = e % NU;
                Ub[e] = uo[q] + ((c < 3) ? vec[3 * k + c] : vec[3 * N + k]);
            }
        }
        for (int e = i; e < N * NK; e += 16) {
            const int k = e / NK, ii = e % NK;
            Xb[(k + 1) * NX + ii] = dxs[(k + 1) * 16 + ii];
        }
    }
    wave_sync();
    double cost = 0.0, nrow = 0.0;
    bool bad = false, bound = false;
    for (int k = i; k <= N; k += 16) {
        const double* xk = Xb + k * NX;
        double Pp[3], dP[3];
        path_eval(C, xk[13], Pp, dP);
        const bool last = (k == N);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double r = (last ? C.sqQ_T[a] : C.sqQ_dt[a]) * C.Sr[a] * (Pp[a] - xk[6 + a]);
            cost += r * r;
        }
        if (!last) {
            const double rv = C.sw * (C.sv * C.vref - C.sv * xk[14]);
            cost += rv * rv;
            for (int c = 0; c < NU; ++c) {
                const double su = C.Su[c] * Ub[k * NU + c];
                cost += C.dt * C.Rraw[c] * su * su;
            }
        }
        for (int ii = 0; ii < NX; ++ii) if (!isfinite(xk[ii])) bad = true;
        if (k < N) for (int c = 0; c < NU; ++c) if (!isfinite(Ub[k * NU + c])) bad = true;
        if (k >= 1)
            for (int ii = 1; ii < 13; ++ii) {
                const double lb = sbnd[ii], ub = sbnd[16 + ii];
                if (xk[ii] < lb - bound_tol(lb) || xk[ii] > ub + bound_tol(ub)) { bound = true; nrow += 1.0; }
            }
    }
    cost = row_sum16(cost);
    nrow = row_sum16(nrow);
    const bool rbad = ((__builtin_amdgcn_ballot_w64(bad) >> (16 * g)) & 0xFFFFull) != 0;
    const bool rbound = ((__builtin_amdgcn_ballot_w64(bound) >> (16 * g)) & 0xFFFFull) != 0;
    if (i == 0) {
        double Pp[3], dP[3];
        path_eval(C, Xb[13], Pp, dP);
        double pe = 0.0;
        for (int a = 0; a < 3; ++a) { const double e = C.Sr[a] * (Pp[a] - Xb[6 + a]); pe += e * e; }
        double* dg = diag + (size_t)b * 6;
        dg[0] = sqrt(pe);
        dg[1] = fabs(C.sv * C.vref - C.sv * Xb[14]);
        dg[2] = cost;
        dg[3] = Xb[13];
        dg[4] = Ub[3];
        dg[5] = kkt;
        // loads before stores again (status and the running sums share a type)
        int32_t st = status[b];
        int32_t acc[4] = {0, 0, 0, 0};
        if (iters_acc) { acc[0] = iters_acc[b]; acc[1] = iters_acc[B + b]; acc[2] = iters_acc[2 * B + b]; acc[3] = iters_in[b]; }
        if (rbad) st |= 1;
        if (!(kkt < 1e-8)) st |= 2;
        if (!accept) st |= 32;
        if (rbound && !rbad) st |= 8;
        status[b] = st;
        if (iters_acc) {                               // running sums since kite_nmpc_timing_start
            iters_acc[b] = acc[0] + acc[3];
            iters_acc[B + b] = acc[1] + ((rbound && !rbad) ? 1 : 0);
            iters_acc[2 * B + b] = acc[2] + (rbad ? 0 : (int32_t)nrow);
        }
        for (int c = 0; c < NU; ++c) u0_out[(size_t)b * NU + c] = Ub[c];
    }
}

size_t qp_split_ckpt_doubles() { return QP_CK_DOUBLES; }
int qp_split_iteration() { return QP_SPLIT_IT; }
bool qp_tiled_supported(const RtiConst& C) { return (C.N == 4 * QP_NTA || C.N == 40) && C.n == 4 * C.N + 2; }

#include "qp_lds.inc"

hipError_t launch_qp_tiled(const ModelConst& P, const RtiConst& C, int B, const double* Htl, const double* Hab,
                           const double* Hbb, const double* hs, const double* Cr, const double* cl,
                           const double* cu, const double* hmax, const double* AB, const double* DEF, double* X,
                           double* U, double* u0, double* diag, int32_t* status, double* kkt, int32_t* iters,
                           const int32_t* order, int32_t* lazy, double* wstep, hipStream_t s,
                           hipEvent_t after_main, const QpSplitBufs* split) {
    const int G = B < QP_LAZY_GRID ? B : QP_LAZY_GRID;
    if (C.N == 4 * QP_NTA) {
        if (split) {
            // first phase -> order of the kites still running by their residual -> second phase
            hipLaunchKernelGGL(k_qp_tiled, dim3(B), dim3(64), 0, s, P, C, B, Htl, Hab, Hbb, hs, Cr, cl, cu,
                               hmax, AB, DEF, X, U, u0, diag, status, kkt, iters, order, lazy, wstep, split->ckpt,
                               split->key);
            const hipError_t er = launch_qp_order_keys(B, QP_KEY_BINS - 1, split->key, split->order2, s);
            if (er != hipSuccess) return er;
            hipLaunchKernelGGL(k_qp_tiled_resume, dim3(B), dim3(64), 0, s, P, C, B, Htl, Hab, Hbb, hs, Cr, cl, cu,
                               hmax, AB, DEF, X, U, u0, diag, status, kkt, iters, split->order2, lazy, wstep,
                               split->ckpt, split->key);
        } else {
            hipLaunchKernelGGL(k_qp_tiled_whole, dim3(B), dim3(64), 0, s, P, C, B, Htl, Hab, Hbb, hs, Cr, cl, cu,
                               hmax, AB, DEF, X, U, u0, diag, status, kkt, iters, order, lazy, wstep);
        }
        if (after_main) { const hipError_t er = hipEventRecord(after_main, s); if (er != hipSuccess) return er; }
        hipLaunchKernelGGL(k_expand20, dim3((B + 3) / 4), dim3(64), 0, s, C, B, wstep, AB, DEF, X, U, u0, diag,
                           status, kkt, iters, iters ? iters + B : nullptr, lazy);
        hipLaunchKernelGGL(k_qp_tiled_lazy, dim3(G), dim3(64), 0, s, P, C, B, Htl, Hab, Hbb, hs, Cr, cl, cu, hmax,
                           AB, DEF, X, U, u0, diag, status, kkt, iters, order, lazy, wstep);
    } else if (C.N == 40) {
        hipLaunchKernelGGL((k_qp_lds<10, 1>), dim3(B), dim3(QL_T), 0, s, P, C, B, Htl, Hab, Hbb, hs, Cr, cl,
                           cu, hmax, AB, DEF, X, U, u0, diag, status, kkt, iters, order, lazy, wstep);
        if (after_main) { const hipError_t er = hipEventRecord(after_main, s); if (er != hipSuccess) return er; }
        hipLaunchKernelGGL((k_qp_lds_lazy<10, 1>), dim3(G), dim3(QL_T), 0, s, P, C, B, Htl, Hab, Hbb, hs, Cr, cl,
                           cu, hmax, AB, DEF, X, U, u0, diag, status, kkt, iters, order, lazy, wstep);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
