// ident_kernels.hip -- batched identification of the 21 aerodynamic
// coefficients from flight logs on gfx950 (kite_identification_test.cpp as a
// Gauss-Newton / Levenberg-Marquardt iteration on the device; the formulation
// is in kite_nmpc.h).
//
// k_ident_accum  the hot path.  Per (kite, chunk of whole segments): the
//   prediction, its forward sensitivities with respect to the 21 through RK4
//   in variational form -- per stage dK = (df/dx) dX + df/dp_j, the first term
//   from kite_rhs<Dual> with dX as the tangent seed, the second analytic
//   (kite_model_dp.hpp) -- and the partial sums of S~'QS~ (upper triangle, 231
//   values), S~'Qe and e'Qe.
//   Lane layout: lanes are directions.  A 64-lane block holds 3 items of 21
//   lanes (lane 63 idles); lane j of an item carries column j of S~, already
//   scaled by s_j.  The 13 x 21 sensitivity of a sample is exchanged through
//   LDS and lane j accumulates column j of the products on VALU (13 x 21
//   multiply-adds per lane and sample).  An item's model constants, formed
//   from its kite_params row and the trial parameters, sit in LDS too.
//   Reduction: no atomics.  An item stores its partials to the workspace slab
//   [kite][chunk][256]; k_ident_solve sums them in ascending chunk order, so a
//   kite's result does not depend on the batch around it.
// k_ident_solve  one block per kite: that sum, the accept / reject decision,
//   the active set, the 21 x 21 Cholesky (lane i owns row i, in LDS), the
//   clipped trial, status and lambda.  With `normal` it stops after the sum and
//   writes A, g and the cost (kite_nmpc_ident_normal).
// k_ident_sens   one sample interval per item: x+ and d x+ / d p (unscaled).
// k_ident_accum_w, k_ident_sens_w  the same bodies (ident_accum_body.inc,
//   ident_sens_body.inc) under a known world-frame wind per sample: the
//   aerodynamics see v_a = v - q^-1 (x) [0,W] (x) q.  Per stage the first term
//   is kite_rhs<Dual, true> (v_a depends on q, whose tangent the Dual carries),
//   the second kite_rhs_dp<true> at v_a (v_a does not depend on the 21).  The
//   sample's wind is three doubles per lane, loaded where the control is.  The
//   windless kernels include the same bodies with WIND = false and are, as
//   compiled, what they were before the wind instances existed.
// k_ident_accum_jw, k_ident_solve24, k_ident_sens_jw  the wind identified
//   jointly with the 21: 24 unknowns, the last three a constant world-frame
//   wind offset w; the model of sample k sees W0[k] + w.  The same bodies a
//   third time (JOINT).  Lane layout: 2 items of 24 lanes per block (lanes
//   48..63 idle).  Lane j < 21 carries column j as in k_ident_accum_w; lane
//   21 + i carries d x^ / d w_i: the wind enters kite_rhs<Dual, true, Dual> as
//   a Dual whose tangent is w_scale on lane 21 + i and 0 on every other lane,
//   and the analytic d f / d p term is multiplied by 0 there.  One instruction
//   stream serves both kinds of lane: a zero tangent adds exact zeros, so
//   columns 0..20 have k_ident_accum_w's values.  The 24 accumulators of a
//   lane live in LDS between samples (the wind kernel already holds 489 of 512
//   registers), the slab is 328 doubles (300 + 24 + 1, padded).
//
// Barriers: the items of a block share every barrier.  No lane returns or
// leaves a loop early, all trip counts are kernel arguments; an out-of-range
// or finished item is predicated, loads zeros and stores nothing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ident_kernels.hpp"
#include "kite_model.hpp"
#include "kite_model_dp.hpp"
#include "kite_nmpc/kite_nmpc.h"

namespace kite {

constexpr int ID_T = 64;              // threads per block
constexpr int ID_ITEMS = 3;           // items of 21 lanes per block
constexpr int ID_LD = NP + 1;         // LDS row stride of a 13 x 21 sensitivity

// the sample interval under the held control for direction j: x (value and
// tangent column j, scaled by sc) advanced by `substeps` RK4 substeps of hs.
// The value part repeats plant_lane's (plant_kernels.hip) stage arithmetic.
// WIND: the sample's world-frame wind wnd[0..2], plain doubles held over the
// interval as u is; WIND = false is the windless interval, instruction for
// instruction.
template <bool WIND>
__device__ __forceinline__ void ident_interval(const ModelConst& P, Dual* x, const double* u, double hs, int substeps,
                                               int j, double sc, const double* wnd = nullptr) {
    Dual ud[NKU];
#pragma unroll
    for (int i = 0; i < NKU; ++i) ud[i] = mk(u[i], 0.0);
#pragma unroll 1
    for (int m = 0; m < substeps; ++m) {
        Dual xs[NK], acc[NK], kv[NK];
#pragma unroll
        for (int i = 0; i < NK; ++i) { xs[i] = x[i]; acc[i] = x[i]; }
#pragma unroll 1
        for (int st = 0; st < 4; ++st) {
            // the model constants are read from LDS in every stage: hoisted out of
            // the loops they would hold 94 registers next to the RK4 state
            asm volatile("" ::: "memory");
            double fp[6];
            if constexpr (WIND) {
                // v_a depends on q, whose tangent the Dual carries; d f / d p_j at v_a
                kite_rhs<Dual, true>(P, xs, ud, kv, wnd);
                double xv[NK];
#pragma unroll
                for (int i = 0; i < NK; ++i) xv[i] = xs[i].v;
                kite_rhs_dp<true>(P, xv, u, j, sc, fp, wnd);
            } else {
                kite_rhs<Dual>(P, xs, ud, kv);
                double xv[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) xv[i] = xs[i].v;
                kite_rhs_dp(P, xv, u, j, sc, fp);
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) kv[i].t += fp[i];
            const double wa = (st == 0 || st == 3) ? hs / 6.0 : hs / 3.0;
            const double wn = (st < 2) ? 0.5 * hs : hs;
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                acc[i].v += wa * kv[i].v;
                acc[i].t += wa * kv[i].t;
                xs[i].v = x[i].v + wn * kv[i].v;
                xs[i].t = x[i].t + wn * kv[i].t;
            }
        }
#pragma unroll
        for (int i = 0; i < NK; ++i) x[i] = acc[i];
    }
}

// lane -> (item of the block, direction); lane 63 belongs to no item
struct IdLane { int it, j; bool on; };
__device__ __forceinline__ IdLane id_lane() {
    const int t = threadIdx.x;
    const int it = t / NP;
    return IdLane{it, t - it * NP, it < ID_ITEMS};
}

// the item's model constants into LDS (lane 0 of the item), and its scale s_j
__device__ __forceinline__ double id_setup(ModelConst* sP, const IdLane& l, bool valid, const double* row,
                                           const double* p21) {
    double sc = 1.0;
    if (valid) {
        const double pr = row[ident_field(l.j)];
        sc = pr != 0.0 ? fabs(pr) : 1.0;
        if (l.j == 0) sP[l.it] = ident_model_const(row, p21);
    }
    return sc;
}

// ---- joint instance: 24 directions, the last three the wind offset ---------------
constexpr int IDJ_ITEMS = 2;          // items of 24 lanes per block

// ident_interval<true> for direction j of 24.  j < 21: column j of the 21, the
// wind's tangent is 0.  j = 21 + i: d / d w_i scaled by sc (= w_scale): the
// wind's tangent is sc e_i and d f / d p is multiplied by 0 (an exact zero for
// finite data).  No lane takes another path than its neighbours.
__device__ __forceinline__ void ident_interval_j(const ModelConst& P, Dual* x, const double* u, double hs,
                                                 int substeps, int j, double sc, const double* wnd) {
    Dual ud[NKU], wd[3];
#pragma unroll
    for (int i = 0; i < NKU; ++i) ud[i] = mk(u[i], 0.0);
#pragma unroll
    for (int i = 0; i < 3; ++i) wd[i] = mk(wnd[i], j == NP + i ? sc : 0.0);
    const int jp = j < NP ? j : 0;
    const double scp = j < NP ? sc : 0.0;
#pragma unroll 1
    for (int m = 0; m < substeps; ++m) {
        Dual xs[NK], acc[NK], kv[NK];
#pragma unroll
        for (int i = 0; i < NK; ++i) { xs[i] = x[i]; acc[i] = x[i]; }
#pragma unroll 1
        for (int st = 0; st < 4; ++st) {
            asm volatile("" ::: "memory");     // the model constants stay in LDS (ident_interval)
            double fp[6];
            kite_rhs<Dual, true, Dual>(P, xs, ud, kv, wd);
            double xv[NK];
#pragma unroll
            for (int i = 0; i < NK; ++i) xv[i] = xs[i].v;
            kite_rhs_dp<true>(P, xv, u, jp, scp, fp, wnd);
#pragma unroll
            for (int i = 0; i < 6; ++i) kv[i].t += fp[i];
            const double wa = (st == 0 || st == 3) ? hs / 6.0 : hs / 3.0;
            const double wn = (st < 2) ? 0.5 * hs : hs;
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                acc[i].v += wa * kv[i].v;
                acc[i].t += wa * kv[i].t;
                xs[i].v = x[i].v + wn * kv[i].v;
                xs[i].t = x[i].t + wn * kv[i].t;
            }
        }
#pragma unroll
        for (int i = 0; i < NK; ++i) x[i] = acc[i];
    }
}

// lane -> (item of the block, direction of 24); lanes 48..63 belong to no item
__device__ __forceinline__ IdLane idj_lane() {
    const int t = threadIdx.x;
    const int it = t / IDJ_NP;
    return IdLane{it, t - it * IDJ_NP, it < IDJ_ITEMS};
}

// id_setup for 24 lanes: the scale of a wind lane is w_scale
__device__ __forceinline__ double idj_setup(ModelConst* sP, const IdLane& l, bool valid, const double* row,
                                            const double* p21, double w_scale) {
    double sc = 1.0;
    if (valid) {
        if (l.j < NP) {
            const double pr = row[ident_field(l.j)];
            sc = pr != 0.0 ? fabs(pr) : 1.0;
        } else {
            sc = w_scale;
        }
        if (l.j == 0) sP[l.it] = ident_model_const(row, p21);
    }
    return sc;
}

// what the body's JOINT branches name, in the kernels where those branches are dead
#define ID_NO_JOINT_ARGS \
    const double* const wj = nullptr; \
    constexpr int w_stride = 0;       \
    double* const sAcc = nullptr;     \
    const IdentWindConst WC{};

__global__ __launch_bounds__(ID_T) void k_ident_accum(IdentConst C, const double* __restrict__ rows,
                                                      const double* __restrict__ p21, int p_stride,
                                                      const double* __restrict__ state,
                                                      const double* __restrict__ X, const double* __restrict__ U,
                                                      double* __restrict__ slab) {
    constexpr bool WIND = false, JOINT = false;
    const double* const W = nullptr;          // no wind log: the body's WIND branches are dead
    ID_NO_JOINT_ARGS
#include "ident_accum_body.inc"
}

__global__ __launch_bounds__(ID_T) void k_ident_accum_w(IdentConst C, const double* __restrict__ rows,
                                                        const double* __restrict__ p21, int p_stride,
                                                        const double* __restrict__ state,
                                                        const double* __restrict__ X, const double* __restrict__ U,
                                                        const double* __restrict__ W, double* __restrict__ slab) {
    constexpr bool WIND = true, JOINT = false;
    ID_NO_JOINT_ARGS
#include "ident_accum_body.inc"
}

__global__ __launch_bounds__(ID_T) void k_ident_accum_jw(IdentConst C, IdentWindConst WC,
                                                         const double* __restrict__ rows,
                                                         const double* __restrict__ p21,
                                                         const double* __restrict__ wj, int p_stride, int w_stride,
                                                         const double* __restrict__ state,
                                                         const double* __restrict__ X, const double* __restrict__ U,
                                                         const double* __restrict__ W, double* __restrict__ slab) {
    constexpr bool WIND = true, JOINT = true;
    __shared__ double sAcc[IDJ_NP * ID_T];
#include "ident_accum_body.inc"
}

__device__ __forceinline__ int id_packed(int i, int j) {      // index of A[i][j] in the packed upper triangle
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return hi * (hi + 1) / 2 + lo;
}

__global__ __launch_bounds__(ID_T) void k_ident_solve(IdentConst C, int first, int normal,
                                                      const double* __restrict__ rows,
                                                      const double* __restrict__ p21,
                                                      const double* __restrict__ slab, double* __restrict__ state,
                                                      double* __restrict__ Aout, double* __restrict__ gout,
                                                      double* __restrict__ cout, double* __restrict__ params_out,
                                                      double* __restrict__ cost2, int32_t* __restrict__ evals,
                                                      int32_t* __restrict__ status) {
    __shared__ double sR[ID_SLAB];            // the chunk sums
    __shared__ double sAA[ID_NA];             // A of the accepted point (packed, without alpha I)
    __shared__ double sM[NP * ID_LD];         // that A + damping, then its Cholesky factor (lower)
    __shared__ double sz[NP], sg[NP], sy[NP], ss[NP];
    __shared__ int sok;
    const int t = threadIdx.x, kite = blockIdx.x;
    const double* row = rows + (size_t)(C.nparams == 1 ? 0 : kite) * 52;
    double* st = state ? state + (size_t)kite * ID_STATE : nullptr;

    // the kite's row is a model (every lane looks at a share of it; uniform)
    bool rok = true;
    if (t < 52) rok = isfinite(row[t]);
    rok = !__any(!rok) && (row[10] > 0.0) && (row[11] * row[13] - row[14] * row[14] != 0.0) && (row[12] != 0.0);

    int flags = 0;
    if (!normal) flags = first ? (rok ? 0 : ID_F_DEAD) : (int)st[ID_S_FLAGS];
    const bool live = normal || (flags & (ID_F_DONE | ID_F_DEAD)) == 0;    // uniform over the block

    // 1. the partial sums in ascending chunk order
    for (int e = t; e < ID_SLAB; e += ID_T) {
        double s = 0.0;
        if (live && e <= ID_SLAB_C)
#pragma unroll 1
            for (int c = 0; c < C.nchunks; ++c) s += slab[((size_t)kite * C.nchunks + c) * ID_SLAB + e];
        sR[e] = s;
    }
    const double pr = t < NP ? row[ident_field(t)] : 0.0;
    const double sc = pr != 0.0 ? fabs(pr) : 1.0;
    double z = 0.0;                            // the point of this evaluation
    if (t < NP) {
        if (normal) z = (p21[(size_t)kite * NP + t] - pr) / sc;
        else if (!first) z = st[ID_S_ZT + t];
        sz[t] = z;
    }
    __syncthreads();
    const double T = (double)C.T;
    double c = sR[ID_SLAB_C] / T;
    {
        double zz = 0.0;
#pragma unroll 1
        for (int i = 0; i < NP; ++i) zz = fma(sz[i], sz[i], zz);
        c += C.alpha * zz;
    }
    const double g = t < NP ? sR[ID_SLAB_G + t] / T - C.alpha * z : 0.0;

    if (normal) {                              // uniform
        if (t < NP) {
#pragma unroll 1
            for (int i = 0; i < NP; ++i)
                Aout[((size_t)kite * NP + i) * NP + t] = sR[id_packed(i, t)] / T + (i == t ? C.alpha : 0.0);
            gout[(size_t)kite * NP + t] = g;
        }
        if (t == 0) {
            cout[kite] = c;
            if (status) status[kite] = (isfinite(c) && rok) ? 0 : KITE_IDENT_NAN;
        }
        return;                                // the whole block
    }

    double lam = first ? C.lm0 : st[ID_S_LAM];
    double c_acc = first ? 0.0 : st[ID_S_CACC];
    double c0 = first ? 0.0 : st[ID_S_C0];
    int nev = first ? 0 : (int)st[ID_S_EVALS];
    double z_acc = (t < NP && !first) ? st[ID_S_ZA + t] : 0.0;
    double g_acc = (t < NP && !first) ? st[ID_S_GA + t] : 0.0;
    double z_trial = z;
    const double lo = t < NP ? -C.lb_rel[t] : 0.0, hi = t < NP ? C.ub_rel[t] : 0.0;

    if (live) {                                // uniform: the barriers below are shared
        ++nev;
        // 2. accept or reject
        const bool accept = isfinite(c) && (!(flags & ID_F_ACC) || c <= c_acc);
        if (accept) {
            if (!(flags & ID_F_ACC)) c0 = c;
            flags |= ID_F_ACC;
            c_acc = c;
            z_acc = z;
            g_acc = g;
            for (int e = t; e < ID_NA; e += ID_T) { sAA[e] = sR[e] / T; st[ID_S_AA + e] = sAA[e]; }
            lam = fmax(lam * 0.25, 1e-12);
        } else {
            if (flags & ID_F_ACC)
                for (int e = t; e < ID_NA; e += ID_T) sAA[e] = st[ID_S_AA + e];
            lam = fmin(8.0 * lam, 1e6);
        }
        __syncthreads();
        if (flags & ID_F_ACC) {                // uniform
            // 3. active set, 4. damped normal equations on the free variables
            const bool act = t < NP && ((z_acc <= lo && g_acc < 0.0) || (z_acc >= hi && g_acc > 0.0));
            if (t < NP) { sy[t] = act ? 1.0 : 0.0; sg[t] = act ? 0.0 : g_acc; }
            __syncthreads();
            double tr = 0.0;
#pragma unroll 1
            for (int i = 0; i < NP; ++i) tr += sAA[id_packed(i, i)] + C.alpha;
            const double damp = lam * tr / (double)NP;
            if (t < NP)
#pragma unroll 1
                for (int i = 0; i < NP; ++i) {
                    double v = sAA[id_packed(t, i)] + (i == t ? C.alpha + damp : 0.0);
                    if (act || sy[i] != 0.0) v = i == t ? 1.0 : 0.0;
                    sM[t * ID_LD + i] = v;
                }
            if (t == 0) sok = 1;
            __syncthreads();
            // Cholesky, right-looking; lane i owns row i
#pragma unroll 1
            for (int k = 0; k < NP; ++k) {
                const double d = sM[k * ID_LD + k];
                const bool pd = d > 0.0 && isfinite(d);
                const double dd = pd ? sqrt(d) : 1.0;
                const double lik = (t < NP && t > k) ? sM[t * ID_LD + k] / dd : 0.0;
                __syncthreads();
                if (t == k) { sM[k * ID_LD + k] = dd; if (!pd) sok = 0; }
                if (t < NP && t > k) sM[t * ID_LD + k] = lik;
                __syncthreads();
                if (t < NP && t > k)
#pragma unroll 1
                    for (int i = k + 1; i <= t; ++i) sM[t * ID_LD + i] -= lik * sM[i * ID_LD + k];
                __syncthreads();
            }
            if (t == 0) {                      // L y = g, L' s = y
#pragma unroll 1
                for (int i = 0; i < NP; ++i) {
                    double v = sg[i];
#pragma unroll 1
                    for (int k = 0; k < i; ++k) v -= sM[i * ID_LD + k] * sy[k];
                    sy[i] = v / sM[i * ID_LD + i];
                }
#pragma unroll 1
                for (int i = NP - 1; i >= 0; --i) {
                    double v = sy[i];
#pragma unroll 1
                    for (int k = i + 1; k < NP; ++k) v -= sM[k * ID_LD + i] * ss[k];
                    ss[i] = v / sM[i * ID_LD + i];
                }
            }
            __syncthreads();
            const bool ok = sok != 0;
            double snorm = 0.0;
#pragma unroll 1
            for (int i = 0; i < NP; ++i) snorm = fmax(snorm, ok ? fabs(ss[i]) : 0.0);
            if (!ok) lam = fmin(8.0 * lam, 1e6);
            // 5. the clipped trial, 6. convergence
            if (t < NP) z_trial = fmin(fmax(z_acc + (ok ? ss[t] : 0.0), lo), hi);
            if (accept && snorm < C.tol) flags |= ID_F_DONE;
        }
    }

    // state, trial and outputs (every call: the last one stands)
    const bool have = (flags & ID_F_ACC) && !(flags & ID_F_DEAD);
    if (t < NP) {
        st[ID_S_ZT + t] = z_trial;
        st[ID_S_PT + t] = pr + sc * z_trial;
        st[ID_S_ZA + t] = z_acc;
        st[ID_S_GA + t] = g_acc;
    }
    if (t == 0) {
        st[ID_S_LAM] = lam; st[ID_S_CACC] = c_acc; st[ID_S_C0] = c0;
        st[ID_S_FLAGS] = (double)flags; st[ID_S_EVALS] = (double)nev;
    }
    if (t < 52) params_out[(size_t)kite * 52 + t] = row[t];
    __syncthreads();                           // the row first, then the 21 over it
    const bool atb = t < NP && have && (z_acc <= lo || z_acc >= hi);
    const bool any_atb = __any(atb);
    if (t < NP && have) params_out[(size_t)kite * 52 + ident_field(t)] = pr + sc * z_acc;
    if (t == 0) {
        if (cost2) { cost2[2 * (size_t)kite] = have ? c0 : NAN; cost2[2 * (size_t)kite + 1] = have ? c_acc : NAN; }
        if (evals) evals[kite] = nev;
        if (status)
            status[kite] = have ? (((flags & ID_F_DONE) ? KITE_IDENT_CONVERGED : 0) | (any_atb ? KITE_IDENT_AT_BOUND : 0))
                                : KITE_IDENT_NAN;
    }
}

__global__ __launch_bounds__(ID_T) void k_ident_sens(int count, int nparams, double hs, int substeps,
                                                     const double* __restrict__ rows,
                                                     const double* __restrict__ x13, const double* __restrict__ u3,
                                                     double* __restrict__ xo, double* __restrict__ S) {
    constexpr bool WIND = false, JOINT = false;
    const double* const w3 = nullptr;
#include "ident_sens_body.inc"
}

__global__ __launch_bounds__(ID_T) void k_ident_sens_w(int count, int nparams, double hs, int substeps,
                                                       const double* __restrict__ rows,
                                                       const double* __restrict__ x13, const double* __restrict__ u3,
                                                       const double* __restrict__ w3,
                                                       double* __restrict__ xo, double* __restrict__ S) {
    constexpr bool WIND = true, JOINT = false;
#include "ident_sens_body.inc"
}

__global__ __launch_bounds__(ID_T) void k_ident_sens_jw(int count, int nparams, double hs, int substeps,
                                                        const double* __restrict__ rows,
                                                        const double* __restrict__ x13, const double* __restrict__ u3,
                                                        const double* __restrict__ w3,
                                                        double* __restrict__ xo, double* __restrict__ S) {
    constexpr bool WIND = true, JOINT = true;
#include "ident_sens_body.inc"
}


// k_ident_solve for n = 24: lane i owns row i; variables 21..23 are the wind
// offset (reference w_prior, scale w_scale, box +-w_box / w_scale, prior weight
// alpha_w).  The same active-set and pivot rules; the damping is lambda tr(A) / 24.
__global__ __launch_bounds__(ID_T) void k_ident_solve24(IdentConst C, IdentWindConst WC, int first, int normal,
                                                        const double* __restrict__ rows,
                                                        const double* __restrict__ p21,
                                                        const double* __restrict__ wj,
                                                        const double* __restrict__ slab, double* __restrict__ state,
                                                        double* __restrict__ Aout, double* __restrict__ gout,
                                                        double* __restrict__ cout, double* __restrict__ params_out,
                                                        double* __restrict__ wind_out, double* __restrict__ cost2,
                                                        int32_t* __restrict__ evals, int32_t* __restrict__ status) {
    constexpr int N = IDJ_NP, LDM = IDJ_NP + 1;
    __shared__ double sR[IDJ_SLAB];           // the chunk sums
    __shared__ double sAA[IDJ_NA];            // A of the accepted point (packed, without the prior terms)
    __shared__ double sM[N * LDM];            // that A + damping, then its Cholesky factor (lower)
    __shared__ double sz[N], sg[N], sy[N], ss[N];
    __shared__ int sok;
    const int t = threadIdx.x, kite = blockIdx.x;
    const double* row = rows + (size_t)(C.nparams == 1 ? 0 : kite) * 52;
    double* st = state ? state + (size_t)kite * IDJ_STATE : nullptr;
    const bool isw = t >= NP && t < N;        // a wind lane

    bool rok = true;
    if (t < 52) rok = isfinite(row[t]);
    rok = !__any(!rok) && (row[10] > 0.0) && (row[11] * row[13] - row[14] * row[14] != 0.0) && (row[12] != 0.0);

    int flags = 0;
    if (!normal) flags = first ? (rok ? 0 : ID_F_DEAD) : (int)st[IDJ_S_FLAGS];
    const bool live = normal || (flags & (ID_F_DONE | ID_F_DEAD)) == 0;    // uniform over the block

    // 1. the partial sums in ascending chunk order
    for (int e = t; e < IDJ_SLAB; e += ID_T) {
        double s = 0.0;
        if (live && e <= IDJ_SLAB_C)
#pragma unroll 1
            for (int c = 0; c < C.nchunks; ++c) s += slab[((size_t)kite * C.nchunks + c) * IDJ_SLAB + e];
        sR[e] = s;
    }
    // reference value, scale and prior weight of variable t
    double pr = 0.0, sc = 1.0, al = 0.0;
    if (t < NP) {
        pr = row[ident_field(t)];
        sc = pr != 0.0 ? fabs(pr) : 1.0;
        al = C.alpha;
    } else if (isw) {
        pr = WC.w_prior[t - NP];
        sc = WC.w_scale;
        al = WC.alpha_w;
    }
    double z = 0.0;                            // the point of this evaluation
    if (t < N) {
        if (normal) z = ((isw ? wj[(size_t)kite * 3 + (t - NP)] : p21[(size_t)kite * NP + t]) - pr) / sc;
        else if (!first) z = st[IDJ_S_ZT + t];
        sz[t] = z;
    }
    __syncthreads();
    const double T = (double)C.T;
    double c = sR[IDJ_SLAB_C] / T;
    {
        double zz = 0.0, zw = 0.0;
#pragma unroll 1
        for (int i = 0; i < NP; ++i) zz = fma(sz[i], sz[i], zz);
#pragma unroll 1
        for (int i = NP; i < N; ++i) zw = fma(sz[i], sz[i], zw);
        c += C.alpha * zz + WC.alpha_w * zw;
    }
    const double g = t < N ? sR[IDJ_SLAB_G + t] / T - al * z : 0.0;

    if (normal) {                              // uniform
        if (t < N) {
#pragma unroll 1
            for (int i = 0; i < N; ++i)
                Aout[((size_t)kite * N + i) * N + t] = sR[id_packed(i, t)] / T + (i == t ? al : 0.0);
            gout[(size_t)kite * N + t] = g;
        }
        if (t == 0) {
            cout[kite] = c;
            if (status) status[kite] = (isfinite(c) && rok) ? 0 : KITE_IDENT_NAN;
        }
        return;                                // the whole block
    }

    double lam = first ? C.lm0 : st[IDJ_S_LAM];
    double c_acc = first ? 0.0 : st[IDJ_S_CACC];
    double c0 = first ? 0.0 : st[IDJ_S_C0];
    int nev = first ? 0 : (int)st[IDJ_S_EVALS];
    double z_acc = (t < N && !first) ? st[IDJ_S_ZA + t] : 0.0;
    double g_acc = (t < N && !first) ? st[IDJ_S_GA + t] : 0.0;
    double z_trial = z;
    double lo = 0.0, hi = 0.0;
    if (t < NP) { lo = -C.lb_rel[t]; hi = C.ub_rel[t]; }
    else if (isw) { hi = WC.w_box[t - NP] / WC.w_scale; lo = -hi; }

    if (live) {                                // uniform: the barriers below are shared
        ++nev;
        // 2. accept or reject
        const bool accept = isfinite(c) && (!(flags & ID_F_ACC) || c <= c_acc);
        if (accept) {
            if (!(flags & ID_F_ACC)) c0 = c;
            flags |= ID_F_ACC;
            c_acc = c;
            z_acc = z;
            g_acc = g;
            for (int e = t; e < IDJ_NA; e += ID_T) { sAA[e] = sR[e] / T; st[IDJ_S_AA + e] = sAA[e]; }
            lam = fmax(lam * 0.25, 1e-12);
        } else {
            if (flags & ID_F_ACC)
                for (int e = t; e < IDJ_NA; e += ID_T) sAA[e] = st[IDJ_S_AA + e];
            lam = fmin(8.0 * lam, 1e6);
        }
        __syncthreads();
        if (flags & ID_F_ACC) {                // uniform
            // 3. active set, 4. damped normal equations on the free variables
            const bool act = t < N && ((z_acc <= lo && g_acc < 0.0) || (z_acc >= hi && g_acc > 0.0));
            if (t < N) { sy[t] = act ? 1.0 : 0.0; sg[t] = act ? 0.0 : g_acc; }
            __syncthreads();
            double tr = 0.0;
#pragma unroll 1
            for (int i = 0; i < N; ++i) tr += sAA[id_packed(i, i)] + (i < NP ? C.alpha : WC.alpha_w);
            const double damp = lam * tr / (double)N;
            if (t < N)
#pragma unroll 1
                for (int i = 0; i < N; ++i) {
                    double v = sAA[id_packed(t, i)] + (i == t ? al + damp : 0.0);
                    if (act || sy[i] != 0.0) v = i == t ? 1.0 : 0.0;
                    sM[t * LDM + i] = v;
                }
            if (t == 0) sok = 1;
            __syncthreads();
            // Cholesky, right-looking; lane i owns row i
#pragma unroll 1
            for (int k = 0; k < N; ++k) {
                const double d = sM[k * LDM + k];
                const bool pd = d > 0.0 && isfinite(d);
                const double dd = pd ? sqrt(d) : 1.0;
                const double lik = (t < N && t > k) ? sM[t * LDM + k] / dd : 0.0;
                __syncthreads();
                if (t == k) { sM[k * LDM + k] = dd; if (!pd) sok = 0; }
                if (t < N && t > k) sM[t * LDM + k] = lik;
                __syncthreads();
                if (t < N && t > k)
#pragma unroll 1
                    for (int i = k + 1; i <= t; ++i) sM[t * LDM + i] -= lik * sM[i * LDM + k];
                __syncthreads();
            }
            if (t == 0) {                      // L y = g, L' s = y
#pragma unroll 1
                for (int i = 0; i < N; ++i) {
                    double v = sg[i];
#pragma unroll 1
                    for (int k = 0; k < i; ++k) v -= sM[i * LDM + k] * sy[k];
                    sy[i] = v / sM[i * LDM + i];
                }
#pragma unroll 1
                for (int i = N - 1; i >= 0; --i) {
                    double v = sy[i];
#pragma unroll 1
                    for (int k = i + 1; k < N; ++k) v -= sM[k * LDM + i] * ss[k];
                    ss[i] = v / sM[i * LDM + i];
                }
            }
            __syncthreads();
            const bool ok = sok != 0;
            double snorm = 0.0;
#pragma unroll 1
            for (int i = 0; i < N; ++i) snorm = fmax(snorm, ok ? fabs(ss[i]) : 0.0);
            if (!ok) lam = fmin(8.0 * lam, 1e6);
            // 5. the clipped trial, 6. convergence
            if (t < N) z_trial = fmin(fmax(z_acc + (ok ? ss[t] : 0.0), lo), hi);
            if (accept && snorm < C.tol) flags |= ID_F_DONE;
        }
    }

    // state, trial and outputs (every call: the last one stands)
    const bool have = (flags & ID_F_ACC) && !(flags & ID_F_DEAD);
    if (t < N) {
        st[IDJ_S_ZT + t] = z_trial;
        st[IDJ_S_PT + t] = pr + sc * z_trial;
        st[IDJ_S_ZA + t] = z_acc;
        st[IDJ_S_GA + t] = g_acc;
    }
    if (t == 0) {
        st[IDJ_S_LAM] = lam; st[IDJ_S_CACC] = c_acc; st[IDJ_S_C0] = c0;
        st[IDJ_S_FLAGS] = (double)flags; st[IDJ_S_EVALS] = (double)nev;
    }
    if (t < 52) params_out[(size_t)kite * 52 + t] = row[t];
    __syncthreads();                           // the row first, then the 21 over it
    const bool onb = t < N && have && (z_acc <= lo || z_acc >= hi);
    const bool any_atb = __any(onb && !isw), any_watb = __any(onb && isw);
    if (t < NP && have) params_out[(size_t)kite * 52 + ident_field(t)] = pr + sc * z_acc;
    if (isw && wind_out) wind_out[(size_t)kite * 3 + (t - NP)] = have ? pr + sc * z_acc : pr;
    if (t == 0) {
        if (cost2) { cost2[2 * (size_t)kite] = have ? c0 : NAN; cost2[2 * (size_t)kite + 1] = have ? c_acc : NAN; }
        if (evals) evals[kite] = nev;
        if (status)
            status[kite] = have ? (((flags & ID_F_DONE) ? KITE_IDENT_CONVERGED : 0) | (any_atb ? KITE_IDENT_AT_BOUND : 0) |
                                   (any_watb ? KITE_IDENT_WIND_AT_BOUND : 0))
                                : KITE_IDENT_NAN;
    }
}

hipError_t launch_ident_accum_jw(const IdentConst& C, const IdentWindConst& WC, const double* rows, const double* p21,
                                 const double* wj, int p_stride, int w_stride, const double* state,
                                 const double* X, const double* U, const double* W0, double* slab, hipStream_t s) {
    const long long items = (long long)C.count * C.nchunks;
    const dim3 grid((unsigned)((items + IDJ_ITEMS - 1) / IDJ_ITEMS));
    hipLaunchKernelGGL(k_ident_accum_jw, grid, dim3(ID_T), 0, s, C, WC, rows, p21, wj, p_stride, w_stride, state, X, U,
                       W0, slab);
    return hipGetLastError();
}

hipError_t launch_ident_solve24(const IdentConst& C, const IdentWindConst& WC, int first, int normal,
                                const double* rows, const double* p21, const double* wj, const double* slab,
                                double* state, double* A, double* g, double* cost, double* params_out,
                                double* wind_out, double* cost2, int32_t* evals, int32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(k_ident_solve24, dim3(C.count), dim3(ID_T), 0, s, C, WC, first, normal, rows, p21, wj, slab,
                       state, A, g, cost, params_out, wind_out, cost2, evals, status);
    return hipGetLastError();
}

hipError_t launch_ident_sens_jw(int count, int nparams, double hs, int substeps, const double* rows,
                                const double* x13, const double* u3, const double* w3, double* xo, double* S,
                                hipStream_t s) {
    const dim3 grid((count + IDJ_ITEMS - 1) / IDJ_ITEMS);
    hipLaunchKernelGGL(k_ident_sens_jw, grid, dim3(ID_T), 0, s, count, nparams, hs, substeps, rows, x13, u3, w3, xo, S);
    return hipGetLastError();
}

hipError_t launch_ident_accum(const IdentConst& C, const double* rows, const double* p21, int p_stride,
                              const double* state, const double* X, const double* U, const double* W, double* slab,
                              hipStream_t s) {
    const long long items = (long long)C.count * C.nchunks;
    const dim3 grid((unsigned)((items + ID_ITEMS - 1) / ID_ITEMS));
    if (W)
        hipLaunchKernelGGL(k_ident_accum_w, grid, dim3(ID_T), 0, s, C, rows, p21, p_stride, state, X, U, W, slab);
    else
        hipLaunchKernelGGL(k_ident_accum, grid, dim3(ID_T), 0, s, C, rows, p21, p_stride, state, X, U, slab);
    return hipGetLastError();
}

hipError_t launch_ident_solve(const IdentConst& C, int first, int normal, const double* rows, const double* p21,
                              const double* slab, double* state, double* A, double* g, double* cost,
                              double* params_out, double* cost2, int32_t* evals, int32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(k_ident_solve, dim3(C.count), dim3(ID_T), 0, s, C, first, normal, rows, p21, slab, state, A, g,
                       cost, params_out, cost2, evals, status);
    return hipGetLastError();
}

hipError_t launch_ident_sens(int count, int nparams, double hs, int substeps, const double* rows, const double* x13,
                             const double* u3, const double* w3, double* xo, double* S, hipStream_t s) {
    const dim3 grid((count + ID_ITEMS - 1) / ID_ITEMS);
    if (w3)
        hipLaunchKernelGGL(k_ident_sens_w, grid, dim3(ID_T), 0, s, count, nparams, hs, substeps, rows, x13, u3, w3, xo,
                           S);
    else
        hipLaunchKernelGGL(k_ident_sens, grid, dim3(ID_T), 0, s, count, nparams, hs, substeps, rows, x13, u3, xo, S);
    return hipGetLastError();
}

}  // namespace kite
