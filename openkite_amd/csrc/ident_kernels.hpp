// ident_kernels.hpp -- internal interface between the C ABI (kite_nmpc.cpp) and
// the identification kernels (ident_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kite_nmpc/kite_nmpc.h"

namespace kite {

// one evaluation's arguments, precomputed on the host from kite_ident_config
struct IdentConst {
    int count, nparams;     // kites; rows of kite_params (1 or count)
    int T, L, substeps;     // samples, samples per segment, RK4 substeps per sample
    int spc, nchunks, pad_; // segments per chunk, chunks per kite
    double hs;              // h / substeps
    double Q[13], alpha, lm0, tol;
    double lb_rel[KITE_IDENT_NP], ub_rel[KITE_IDENT_NP];
};

// workspace slab of one (kite, chunk): A's upper triangle packed by columns
// (231), S~'Qe (21), e'Qe (1), padded to 256 doubles
constexpr int ID_NA = KITE_IDENT_NP * (KITE_IDENT_NP + 1) / 2;
constexpr int ID_SLAB_G = ID_NA, ID_SLAB_C = ID_NA + KITE_IDENT_NP, ID_SLAB = 256;
// iteration state of one kite (doubles): trial z and p, accepted z, g and A
// (packed, without alpha I), accepted and first cost, lambda, flags, evaluations
constexpr int ID_S_ZT = 0, ID_S_PT = 21, ID_S_ZA = 42, ID_S_GA = 63, ID_S_AA = 84;
constexpr int ID_S_CACC = ID_S_AA + ID_NA, ID_S_LAM = ID_S_CACC + 1, ID_S_C0 = ID_S_CACC + 2;
constexpr int ID_S_FLAGS = ID_S_CACC + 3, ID_S_EVALS = ID_S_CACC + 4, ID_STATE = 320;
static_assert(ID_S_EVALS < ID_STATE, "state layout");
constexpr int ID_F_ACC = 1;     // some evaluation was accepted
constexpr int ID_F_DONE = 2;    // converged
constexpr int ID_F_DEAD = 4;    // the row is no model

// rows: nparams x 52 (kite_params); p21: parameter values of the evaluation,
// kite b's at p21 + b p_stride, or nullptr (the rows' own); state: nullptr or
// the iteration state (finished kites are skipped); slab: count x nchunks x ID_SLAB;
// W: the wind log count x T x 3 (k_ident_accum_w), or nullptr (k_ident_accum)
hipError_t launch_ident_accum(const IdentConst& C, const double* rows, const double* p21, int p_stride,
                              const double* state, const double* X, const double* U, const double* W, double* slab,
                              hipStream_t s);
// normal: A (count x 21 x 21), g, cost, status at p21 (count x 21) from the slab;
// otherwise one iteration on `state` (first: initialise it), and the outputs
hipError_t launch_ident_solve(const IdentConst& C, int first, int normal, const double* rows, const double* p21,
                              const double* slab, double* state, double* A, double* g, double* cost,
                              double* params_out, double* cost2, int32_t* evals, int32_t* status, hipStream_t s);
// w3: the items' wind count x 3 (k_ident_sens_w), or nullptr (k_ident_sens)
hipError_t launch_ident_sens(int count, int nparams, double hs, int substeps, const double* rows, const double* x13,
                             const double* u3, const double* w3, double* xo, double* S, hipStream_t s);

// ---- the wind identified jointly with the 21 (k_ident_accum_jw, k_ident_solve24,
// k_ident_sens_jw): 24 variables, the last three the wind offset w
constexpr int IDJ_NP = KITE_IDENT_NPW;
struct IdentWindConst {
    double w_scale, w_prior[3], w_box[3], alpha_w;
};
// slab of one (kite, chunk): A's upper triangle (300), S~'Qe (24), e'Qe (1), padded to 328
constexpr int IDJ_NA = IDJ_NP * (IDJ_NP + 1) / 2;
constexpr int IDJ_SLAB_G = IDJ_NA, IDJ_SLAB_C = IDJ_NA + IDJ_NP, IDJ_SLAB = 328;
// iteration state of one kite, as ID_S_* with 24 entries per vector; PT holds
// the trial's 21 parameter values and its wind offset
constexpr int IDJ_S_ZT = 0, IDJ_S_PT = 24, IDJ_S_ZA = 48, IDJ_S_GA = 72, IDJ_S_AA = 96;
constexpr int IDJ_S_CACC = IDJ_S_AA + IDJ_NA, IDJ_S_LAM = IDJ_S_CACC + 1, IDJ_S_C0 = IDJ_S_CACC + 2;
constexpr int IDJ_S_FLAGS = IDJ_S_CACC + 3, IDJ_S_EVALS = IDJ_S_CACC + 4, IDJ_STATE = 408;
static_assert(IDJ_S_EVALS < IDJ_STATE && IDJ_SLAB_C < IDJ_SLAB, "joint layouts");

// p21 / wj: the evaluation's parameter values and wind offset, kite b's at
// p21 + b p_stride and wj + b w_stride, or nullptr (the rows' own, w_prior);
// W0: the known wind log count x T x 3 or nullptr (zeros); slab: count x nchunks x IDJ_SLAB
hipError_t launch_ident_accum_jw(const IdentConst& C, const IdentWindConst& WC, const double* rows, const double* p21,
                                 const double* wj, int p_stride, int w_stride, const double* state,
                                 const double* X, const double* U, const double* W0, double* slab, hipStream_t s);
// normal: A (count x 24 x 24), g, cost, status at (p21 count x 21, wj count x 3);
// otherwise one iteration on `state`, the outputs, and wind_out count x 3
hipError_t launch_ident_solve24(const IdentConst& C, const IdentWindConst& WC, int first, int normal,
                                const double* rows, const double* p21, const double* wj, const double* slab,
                                double* state, double* A, double* g, double* cost, double* params_out,
                                double* wind_out, double* cost2, int32_t* evals, int32_t* status, hipStream_t s);
// w3: the items' total wind count x 3; S count x 13 x 24
hipError_t launch_ident_sens_jw(int count, int nparams, double hs, int substeps, const double* rows,
                                const double* x13, const double* u3, const double* w3, double* xo, double* S,
                                hipStream_t s);

}  // namespace kite
