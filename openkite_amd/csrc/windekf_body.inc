// windekf_body.inc -- the body of k_ekf_wind (windekf_kernels.hip), included
// by its homogeneous and its per-kite instance so that both execute the same
// arithmetic and walk the same barriers.  In scope: P (ModelConst: the kernel
// argument, or the kite's table row), b, kk, j, kite (b < count), dt,
// substeps, x, u, Pc, z, W, V, status.
    __shared__ double sA[4 * WEKF_KS];
    __shared__ double sN[4 * WEKF_KS];
    double* sa = sA + kk * WEKF_KS;
    double* sn = sN + kk * WEKF_KS;
    const double h = dt / (double)substeps;

    // xv: [x13 | W3], every lane of the kite holds all of it; pcol: column j of P
    double xv[WEKF_N], uv[NKU], pcol[WEKF_N], wcol[WEKF_N];
    for (int i = 0; i < WEKF_N; ++i) xv[i] = kite ? x[(size_t)b * WEKF_N + i] : 0.0;
    for (int i = 0; i < NKU; ++i) uv[i] = kite ? u[(size_t)b * NKU + i] : 0.0;
    for (int i = 0; i < WEKF_N; ++i) pcol[i] = kite ? Pc[((size_t)b * WEKF_N + i) * WEKF_N + j] : 0.0;
    for (int i = 0; i < WEKF_N; ++i) wcol[i] = W[i * WEKF_N + j];

    bool fin = true;
    for (int i = 0; i < WEKF_N; ++i) fin = fin && isfinite(xv[i]) && isfinite(pcol[i]);
    bool alive = !kite_any(!fin, kk);         // uniform over the kite's lanes
    const bool entry_ok = alive;
    int32_t flag = alive ? 0 : KITE_EKF_NAN;

#pragma unroll 1
    for (int s = 0; s < substeps; ++s) {
        // column j of A = I + J h at the estimate; rows 13..15: W_dot = 0
        {
            double jc[NK];
            wind_jac_col(P, xv, uv, xv + NK, j, jc);
            for (int i = 0; i < NK; ++i) sa[i * WEKF_LD + j] = jc[i] * h + (i == j ? 1.0 : 0.0);
            for (int i = NK; i < WEKF_N; ++i) sa[i * WEKF_LD + j] = (i == j ? 1.0 : 0.0);
        }
        // x13+ = one RK4 step over h under the estimated wind (every lane of the kite)
        double xn[NK];
        {
            double k[NK], xs[NK];
            for (int i = 0; i < NK; ++i) { xn[i] = xv[i]; xs[i] = xv[i]; }
#pragma unroll 1
            for (int st = 0; st < 4; ++st) {
                kite_rhs<double, true>(P, xs, uv, k, xv + NK);
                const double wa = (st == 0 || st == 3) ? h / 6.0 : h / 3.0;
                const double wn = (st < 2) ? 0.5 * h : h;
                for (int i = 0; i < NK; ++i) { xn[i] += wa * k[i]; xs[i] = xv[i] + wn * k[i]; }
            }
        }
        __syncthreads();
        // (A P)[:, j]
        for (int i = 0; i < WEKF_N; ++i) {
            double t = 0.0;
            for (int k = 0; k < WEKF_N; ++k) t = fma(sa[i * WEKF_LD + k], pcol[k], t);
            sn[i * WEKF_LD + j] = t;
        }
        __syncthreads();
        // P+[:, j] = sum_k (A P)[:, k] A[j][k] + Wcov[:, j]
        double pn[WEKF_N];
        for (int i = 0; i < WEKF_N; ++i) {
            double t = wcol[i];
            for (int k = 0; k < WEKF_N; ++k) t = fma(sn[i * WEKF_LD + k], sa[j * WEKF_LD + k], t);
            pn[i] = t;
        }
        bool ok = true;
        for (int i = 0; i < NK; ++i) ok = ok && isfinite(xn[i]);
        for (int i = 0; i < WEKF_N; ++i) ok = ok && isfinite(pn[i]);
        const bool bad = kite_any(!ok, kk);
        if (alive && bad) { alive = false; flag = KITE_EKF_NAN; }   // keeps the last finite x16, P
        if (alive) {
            for (int i = 0; i < NK; ++i) xv[i] = xn[i];
            for (int i = 0; i < WEKF_N; ++i) pcol[i] = pn[i];
        }
        __syncthreads();                     // sa, sn are rewritten by the next substep
    }

    if (z) {                                 // uniform over the grid
        for (int i = 0; i < WEKF_N; ++i) sn[i * WEKF_LD + j] = pcol[i];
        __syncthreads();
        // the pose update: ekf_update.hpp
        double L[7][7];
        const bool pd = ekf_chol7<WEKF_LD>(sn, V, kite, L);
        double pu[WEKF_N], xu[WEKF_N], y[7];
        ekf_cov_update<WEKF_N, WEKF_LD>(sn, L, pcol, pu);
        for (int a = 0; a < 7; ++a) y[a] = (kite ? z[(size_t)b * 7 + a] : 0.0) - xv[6 + a];
        ekf_state_update<WEKF_N, WEKF_LD>(sn, L, xv, y, xu);
        // The containment tail, ekf_commit's statements (the reason for the
        // symmetrisation is written there).  This filter keeps its own copy:
        // through ekf_commit k_ekf_wind_pk is scheduled 1.2 % slower.
        bool ok = true;
        for (int i = 0; i < WEKF_N; ++i) ok = ok && isfinite(pu[i]) && isfinite(xu[i]);
        const bool bad = kite_any(!ok, kk);
        if (alive && !pd) flag |= KITE_EKF_S_NOT_PD;            // update skipped
        else if (alive && bad) flag |= KITE_EKF_NAN;            // keeps the propagated estimate
        const bool updated = alive && pd && !bad;
        if (updated) {
            for (int i = 0; i < WEKF_N; ++i) { pcol[i] = pu[i]; xv[i] = xu[i]; }
        }
        // P <- (P + P') / 2 of an updated kite
        __syncthreads();                     // every lane is done with P+ in sn
        for (int i = 0; i < WEKF_N; ++i) sn[i * WEKF_LD + j] = pcol[i];
        __syncthreads();
        if (updated)
            for (int i = 0; i < WEKF_N; ++i) pcol[i] = 0.5 * (pcol[i] + sn[j * WEKF_LD + i]);
    }
    // a kite that was non-finite on entry is left untouched; one frozen in a
    // substep stores the last finite x16 and P it holds
    if (kite && entry_ok)
        for (int i = 0; i < WEKF_N; ++i) Pc[((size_t)b * WEKF_N + i) * WEKF_N + j] = pcol[i];
    if (kite && entry_ok && j == 0)
        for (int i = 0; i < WEKF_N; ++i) x[(size_t)b * WEKF_N + i] = xv[i];
    if (kite && j == 0 && status) status[b] = flag;
