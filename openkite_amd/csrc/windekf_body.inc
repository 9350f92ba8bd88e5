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
        // S = P+[6:13, 6:13] + V, Cholesky in registers (lower), every lane its own copy
        double L[7][7];
        for (int a = 0; a < 7; ++a)
            for (int c = 0; c <= a; ++c) L[a][c] = kite ? sn[(6 + a) * WEKF_LD + 6 + c] + V[a * 7 + c] : (a == c);
        bool pd = true;
        for (int c = 0; c < 7; ++c) {
            double d = L[c][c];
            for (int k = 0; k < c; ++k) d -= L[c][k] * L[c][k];
            pd = pd && (d > 0.0) && isfinite(d);
            d = sqrt(d);
            L[c][c] = d;
            for (int a = c + 1; a < 7; ++a) {
                double t = L[a][c];
                for (int k = 0; k < c; ++k) t -= L[a][k] * L[c][k];
                L[a][c] = t / d;
            }
        }
        auto solve = [&](double r[7]) {          // r <- S^-1 r
            for (int a = 0; a < 7; ++a) {
                double t = r[a];
                for (int k = 0; k < a; ++k) t -= L[a][k] * r[k];
                r[a] = t / L[a][a];
            }
            for (int a = 6; a >= 0; --a) {
                double t = r[a];
                for (int k = a + 1; k < 7; ++k) t -= L[k][a] * r[k];
                r[a] = t / L[a][a];
            }
        };
        // P[:, j] = P+[:, j] - P+[:, 6:13] S^-1 P+[6:13, j]
        double pu[WEKF_N], xu[WEKF_N];
        {
            double c7[7];
            for (int a = 0; a < 7; ++a) c7[a] = pcol[6 + a];
            solve(c7);
            for (int i = 0; i < WEKF_N; ++i) {
                double t = pcol[i];
                for (int a = 0; a < 7; ++a) t = fma(-sn[i * WEKF_LD + 6 + a], c7[a], t);
                pu[i] = t;
            }
        }
        // x = x+ + P+[:, 6:13] S^-1 (z - x+[6:13])
        {
            double y[7];
            for (int a = 0; a < 7; ++a) y[a] = (kite ? z[(size_t)b * 7 + a] : 0.0) - xv[6 + a];
            solve(y);
            for (int i = 0; i < WEKF_N; ++i) {
                double t = xv[i];
                for (int a = 0; a < 7; ++a) t = fma(sn[i * WEKF_LD + 6 + a], y[a], t);
                xu[i] = t;
            }
        }
        bool ok = true;
        for (int i = 0; i < WEKF_N; ++i) ok = ok && isfinite(pu[i]) && isfinite(xu[i]);
        const bool bad = kite_any(!ok, kk);
        if (alive && !pd) flag |= KITE_EKF_S_NOT_PD;            // update skipped
        else if (alive && bad) flag |= KITE_EKF_NAN;            // keeps the propagated estimate
        const bool updated = alive && pd && !bad;
        if (updated) {
            for (int i = 0; i < WEKF_N; ++i) { pcol[i] = pu[i]; xv[i] = xu[i]; }
        }
        // P <- (P + P') / 2 of an updated kite.  S is factored from its lower
        // triangle alone, so the update does not damp an antisymmetric part of
        // P: rounding seeds one and every further update multiplies it (by 1.4
        // to 1.6 per period in the open-loop run of the tests: 1e-15 becomes
        // 1e-10 within 40 periods and O(1) within 100).  Both halves of a pair
        // add the same two numbers, so P leaves exactly symmetric.
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
