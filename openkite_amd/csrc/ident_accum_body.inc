// ident_accum_body.inc -- the body of k_ident_accum (ident_kernels.hip), included
// by its windless, its wind and its joint instance so that all walk the same
// loops and barriers, and the windless and wind ones stay the kernels they were.
// In scope: WIND, JOINT (constexpr bool), C, rows, p21, p_stride, state, X, U,
// slab, and with WIND the wind log W [count][T][3], row k held over sample
// interval k as U[k] is.  With JOINT (k_ident_accum_jw; WIND is true, W may be
// nullptr = zeros): 24 directions per item and 2 items per block, the wind
// offset wj (kite b's at wj + b w_stride; nullptr: WC.w_prior), the wind
// constants WC, and sAcc, the lanes' 24 accumulators in LDS (entry i of lane t
// at sAcc[i * ID_T + t]): they are in registers only while a sample's products
// are added, not across the interval.
    constexpr int NJ = JOINT ? IDJ_NP : NP;                  // directions = lanes per item
    constexpr int NIT = JOINT ? IDJ_ITEMS : ID_ITEMS;        // items per block
    constexpr int LD = NJ + 1;                               // LDS row stride of a 13 x NJ sensitivity
    constexpr int SLB = JOINT ? IDJ_SLAB : ID_SLAB, SLB_G = JOINT ? IDJ_SLAB_G : ID_SLAB_G;
    constexpr int SLB_C = JOINT ? IDJ_SLAB_C : ID_SLAB_C;
    constexpr int STT = JOINT ? IDJ_STATE : ID_STATE, STT_FLAGS = JOINT ? IDJ_S_FLAGS : ID_S_FLAGS;
    __shared__ ModelConst sP[NIT + 1];
    __shared__ double sS[(NIT + 1) * NK * LD];
    const IdLane l = JOINT ? idj_lane() : id_lane();
    const long long item = (long long)blockIdx.x * NIT + l.it;
    const int kite = (int)(item / C.nchunks), chunk = (int)(item - (long long)kite * C.nchunks);
    bool valid = l.on && kite < C.count;
    // a kite that is finished (converged, or its row is no model) does no further work
    if (valid && state) valid = ((int)state[(size_t)kite * STT + STT_FLAGS] & (ID_F_DONE | ID_F_DEAD)) == 0;
    const double* row = rows + (size_t)(C.nparams == 1 ? 0 : (valid ? kite : 0)) * 52;
    const double* const pk = p21 ? p21 + (size_t)(valid ? kite : 0) * p_stride : nullptr;
    const double sc = JOINT ? idj_setup(sP, l, valid, row, pk, WC.w_scale) : id_setup(sP, l, valid, row, pk);
    __syncthreads();
    const ModelConst& P = sP[l.it];
    double* sm = sS + l.it * NK * LD;
    const double* Xk = X + (size_t)(valid ? kite : 0) * (C.T + 1) * NK;
    const double* Uk = U + (size_t)(valid ? kite : 0) * C.T * NKU;
    const double* Wk = nullptr;
    if constexpr (WIND) Wk = W + (size_t)(valid ? kite : 0) * C.T * 3;

    double aA[NP], ag = 0.0, ac = 0.0;
    double wo[3] = {0.0, 0.0, 0.0};          // JOINT: the item's wind offset w
    if constexpr (JOINT) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            wo[i] = valid ? (wj ? wj[(size_t)kite * w_stride + i] : WC.w_prior[i]) : 0.0;
#pragma unroll
        for (int i = 0; i < NJ; ++i) sAcc[i * ID_T + threadIdx.x] = 0.0;
    } else {
#pragma unroll
        for (int i = 0; i < NP; ++i) aA[i] = 0.0;
    }

    if (__any(valid)) {                      // uniform over the block (one wavefront)
#pragma unroll 1
        for (int sg = 0; sg < C.spc; ++sg) {
            const long long k0 = ((long long)chunk * C.spc + sg) * C.L;
            const bool sv = valid && k0 < C.T;
            Dual x[NK];
#pragma unroll
            for (int i = 0; i < NK; ++i) x[i] = mk(sv ? Xk[(size_t)k0 * NK + i] : 0.0, 0.0);
#pragma unroll 1
            for (int a = 0; a < C.L; ++a) {
                const long long k = k0 + a;
                const bool on = sv && k < C.T;
                double u[NKU];
#pragma unroll
                for (int i = 0; i < NKU; ++i) u[i] = on ? Uk[(size_t)k * NKU + i] : 0.0;
                if constexpr (JOINT) {
                    double wn[3];            // the sample's wind W0[k] + w
#pragma unroll
                    for (int i = 0; i < 3; ++i) wn[i] = ((on && W) ? Wk[(size_t)k * 3 + i] : 0.0) + wo[i];
                    ident_interval_j(P, x, u, C.hs, C.substeps, l.j, sc, wn);
                } else if constexpr (WIND) {
                    double wn[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) wn[i] = on ? Wk[(size_t)k * 3 + i] : 0.0;
                    ident_interval<true>(P, x, u, C.hs, C.substeps, l.j, sc, wn);
                } else {
                    ident_interval<false>(P, x, u, C.hs, C.substeps, l.j, sc);
                }
                // column j of S~ and (lane 0) the residual e into LDS: row r holds
                // S~[r][0..NJ-1] and e_r
#pragma unroll
                for (int r = 0; r < NK; ++r) sm[r * LD + l.j] = x[r].t;
                if (l.j == 0)
#pragma unroll
                    for (int r = 0; r < NK; ++r) sm[r * LD + NJ] = on ? Xk[(size_t)(k + 1) * NK + r] - x[r].v : 0.0;
                __syncthreads();
                if constexpr (JOINT) {
                    double aJ[NJ];
#pragma unroll
                    for (int i = 0; i < NJ; ++i) aJ[i] = sAcc[i * ID_T + threadIdx.x];
                    if (on) {
#pragma unroll 1
                        for (int r = 0; r < NK; ++r) {
                            const double* sr = sm + r * LD;
                            const double e = sr[NJ], q = C.Q[r];
                            const double qe = q * e;
                            const double t = q * sr[l.j];
                            ac = fma(qe, e, ac);
                            ag = fma(sr[l.j], qe, ag);
#pragma unroll
                            for (int i = 0; i < NJ; ++i) aJ[i] = fma(sr[i], t, aJ[i]);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < NJ; ++i) sAcc[i * ID_T + threadIdx.x] = aJ[i];
                } else {
                    if (on) {
#pragma unroll 1
                        for (int r = 0; r < NK; ++r) {
                            const double* sr = sm + r * LD;
                            const double e = sr[NP], q = C.Q[r];
                            const double qe = q * e;
                            const double t = q * sr[l.j];
                            ac = fma(qe, e, ac);
                            ag = fma(sr[l.j], qe, ag);
#pragma unroll
                            for (int i = 0; i < NP; ++i) aA[i] = fma(sr[i], t, aA[i]);
                        }
                    }
                }
                __syncthreads();             // sm is rewritten by the next sample
            }
        }
    }
    if (valid) {
        double* out = slab + ((size_t)kite * C.nchunks + chunk) * SLB;
        const int base = l.j * (l.j + 1) / 2;            // A[i][j], i <= j, packed by columns
        if constexpr (JOINT) {
#pragma unroll
            for (int i = 0; i < NJ; ++i)
                if (i <= l.j) out[base + i] = sAcc[i * ID_T + threadIdx.x];
        } else {
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (i <= l.j) out[base + i] = aA[i];
        }
        out[SLB_G + l.j] = ag;
        if (l.j == 0) out[SLB_C] = ac;
    }
