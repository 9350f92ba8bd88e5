// ident_sens_body.inc -- the body of k_ident_sens (ident_kernels.hip), included
// by its windless, its wind and its joint instance.  In scope: WIND, JOINT
// (constexpr bool), count, nparams, hs, substeps, rows, x13, u3, xo, S, and the
// items' wind w3 [count][3] (nullptr in the windless kernel).  With JOINT
// (k_ident_sens_jw): 24 directions per item, 2 items per block, S 13 x 24.
    constexpr int NJ = JOINT ? IDJ_NP : NP;
    constexpr int NIT = JOINT ? IDJ_ITEMS : ID_ITEMS;
    __shared__ ModelConst sP[NIT + 1];
    const IdLane l = JOINT ? idj_lane() : id_lane();
    const long long item = (long long)blockIdx.x * NIT + l.it;
    const bool valid = l.on && item < count;
    const size_t b = valid ? (size_t)item : 0;
    const double* row = rows + (nparams == 1 ? 0 : b) * 52;
    if constexpr (JOINT) idj_setup(sP, l, valid, row, nullptr, 1.0);
    else id_setup(sP, l, valid, row, nullptr);
    __syncthreads();
    Dual x[NK];
    double u[NKU];
#pragma unroll
    for (int i = 0; i < NK; ++i) x[i] = mk(valid ? x13[b * NK + i] : 0.0, 0.0);
#pragma unroll
    for (int i = 0; i < NKU; ++i) u[i] = valid ? u3[b * NKU + i] : 0.0;
    if constexpr (WIND) {
        double wn[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) wn[i] = valid ? w3[b * 3 + i] : 0.0;
        if constexpr (JOINT) ident_interval_j(sP[l.it], x, u, hs, substeps, l.j, 1.0, wn);
        else ident_interval<true>(sP[l.it], x, u, hs, substeps, l.j, 1.0, wn);
    } else {
        ident_interval<false>(sP[l.it], x, u, hs, substeps, l.j, 1.0);
    }
    if (valid) {
#pragma unroll
        for (int r = 0; r < NK; ++r) S[(b * NK + r) * NJ + l.j] = x[r].t;
        if (l.j == 0)
#pragma unroll
            for (int r = 0; r < NK; ++r) xo[b * NK + r] = x[r].v;
    }
