// ident_accum_body.inc -- the body of k_ident_accum (ident_kernels.hip), included
// by its windless and its wind instance so that both walk the same loops and
// barriers, and the windless one stays the kernel it was.  In scope: WIND
// (constexpr bool), C, rows, p21, p_stride, state, X, U, slab, and with WIND the
// wind log W [count][T][3], row k held over sample interval k as U[k] is.
    __shared__ ModelConst sP[ID_ITEMS + 1];
    __shared__ double sS[(ID_ITEMS + 1) * NK * ID_LD];
    const IdLane l = id_lane();
    const long long item = (long long)blockIdx.x * ID_ITEMS + l.it;
    const int kite = (int)(item / C.nchunks), chunk = (int)(item - (long long)kite * C.nchunks);
    bool valid = l.on && kite < C.count;
    // a kite that is finished (converged, or its row is no model) does no further work
    if (valid && state) valid = ((int)state[(size_t)kite * ID_STATE + ID_S_FLAGS] & (ID_F_DONE | ID_F_DEAD)) == 0;
    const double* row = rows + (size_t)(C.nparams == 1 ? 0 : (valid ? kite : 0)) * 52;
    const double sc = id_setup(sP, l, valid, row, p21 ? p21 + (size_t)(valid ? kite : 0) * p_stride : nullptr);
    __syncthreads();
    const ModelConst& P = sP[l.it];
    double* sm = sS + l.it * NK * ID_LD;
    const double* Xk = X + (size_t)(valid ? kite : 0) * (C.T + 1) * NK;
    const double* Uk = U + (size_t)(valid ? kite : 0) * C.T * NKU;
    const double* Wk = nullptr;
    if constexpr (WIND) Wk = W + (size_t)(valid ? kite : 0) * C.T * 3;

    double aA[NP], ag = 0.0, ac = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) aA[i] = 0.0;

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
                if constexpr (WIND) {
                    double wn[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) wn[i] = on ? Wk[(size_t)k * 3 + i] : 0.0;
                    ident_interval<true>(P, x, u, C.hs, C.substeps, l.j, sc, wn);
                } else {
                    ident_interval<false>(P, x, u, C.hs, C.substeps, l.j, sc);
                }
                // column j of S~ and (lane 0) the residual e into LDS: row r holds
                // S~[r][0..20] and e_r
#pragma unroll
                for (int r = 0; r < NK; ++r) sm[r * ID_LD + l.j] = x[r].t;
                if (l.j == 0)
#pragma unroll
                    for (int r = 0; r < NK; ++r) sm[r * ID_LD + NP] = on ? Xk[(size_t)(k + 1) * NK + r] - x[r].v : 0.0;
                __syncthreads();
                if (on) {
#pragma unroll 1
                    for (int r = 0; r < NK; ++r) {
                        const double* sr = sm + r * ID_LD;
                        const double e = sr[NP], q = C.Q[r];
                        const double qe = q * e;
                        const double t = q * sr[l.j];
                        ac = fma(qe, e, ac);
                        ag = fma(sr[l.j], qe, ag);
#pragma unroll
                        for (int i = 0; i < NP; ++i) aA[i] = fma(sr[i], t, aA[i]);
                    }
                }
                __syncthreads();             // sm is rewritten by the next sample
            }
        }
    }
    if (valid) {
        double* out = slab + ((size_t)kite * C.nchunks + chunk) * ID_SLAB;
        const int base = l.j * (l.j + 1) / 2;            // A[i][j], i <= j, packed by columns
#pragma unroll
        for (int i = 0; i < NP; ++i)
            if (i <= l.j) out[base + i] = aA[i];
        out[ID_SLAB_G + l.j] = ag;
        if (l.j == 0) out[ID_SLAB_C] = ac;
    }
