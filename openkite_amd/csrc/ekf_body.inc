// ekf_body.inc -- the body of k_ekf (ekf_kernels.hip), included by its
// homogeneous and its per-kite instance so that both execute the same
// arithmetic.  In scope: P (ModelConst: the kernel argument, or the kite's
// table row), b, kk, j, kite (b < count), dt, x, u, Pc, z, W, V.
    __shared__ double sA[4][NK * EKF_LD];
    __shared__ double sN[4][NK * EKF_LD];
    const bool col = kite && j < NK;
    double* sa = sA[kk];
    double* sn = sN[kk];

    double xv[NK], uv[NKU];
    for (int i = 0; i < NK; ++i) xv[i] = kite ? x[(size_t)b * NK + i] : 0.0;
    for (int i = 0; i < NKU; ++i) uv[i] = kite ? u[(size_t)b * NKU + i] : 0.0;

    // column j of A = I + J dt at the estimate (kiteEKF.cpp:93)
    if (col) {
        Dual xx[NK], uu[NKU], ff[NK];
        for (int i = 0; i < NK; ++i) xx[i] = mk(xv[i], i == j ? 1.0 : 0.0);
        for (int i = 0; i < NKU; ++i) uu[i] = mk(uv[i], 0.0);
        kite_rhs<Dual>(P, xx, uu, ff);
        for (int i = 0; i < NK; ++i) sa[i * EKF_LD + j] = ff[i].t * dt + (i == j ? 1.0 : 0.0);
    }
    // x+ = one RK4 step over dt (kitemath.cpp:36-51), every lane of the kite
    double xn[NK];
    {
        double k[NK], xs[NK];
        for (int i = 0; i < NK; ++i) { xn[i] = xv[i]; xs[i] = xv[i]; }
#pragma unroll 1
        for (int st = 0; st < 4; ++st) {
            kite_rhs<double>(P, xs, uv, k);
            const double wa = (st == 0 || st == 3) ? dt / 6.0 : dt / 3.0;
            const double wn = (st < 2) ? 0.5 * dt : dt;
            for (int i = 0; i < NK; ++i) { xn[i] += wa * k[i]; xs[i] = xv[i] + wn * k[i]; }
        }
    }
    double pcol[NK];
    for (int i = 0; i < NK; ++i) pcol[i] = col ? Pc[((size_t)b * NK + i) * NK + j] : 0.0;
    __syncthreads();
    // (A P)[:, j]
    if (col) {
        for (int i = 0; i < NK; ++i) {
            double t = 0.0;
            for (int k = 0; k < NK; ++k) t = fma(sa[i * EKF_LD + k], pcol[k], t);
            sn[i * EKF_LD + j] = t;
        }
    }
    __syncthreads();
    // P+[:, j] = sum_k (A P)[:, k] A[j][k] + W[:, j]
    if (col) {
        for (int i = 0; i < NK; ++i) {
            double t = W[i * NK + j];
            for (int k = 0; k < NK; ++k) t = fma(sn[i * EKF_LD + k], sa[j * EKF_LD + k], t);
            pcol[i] = t;
        }
    }
    if (z) {
        __syncthreads();
        if (col) for (int i = 0; i < NK; ++i) sn[i * EKF_LD + j] = pcol[i];
        __syncthreads();
        // S = P+[6:13, 6:13] + V, Cholesky in registers (ekf_update.hpp); the
        // pivots are not checked here
        double L[7][7];
        ekf_chol7<EKF_LD>(sn, V, kite, L);
        // P[:, j] = P+[:, j] - P+[:, 6:13] S^-1 P+[6:13, j]
        if (col) ekf_cov_update<NK, EKF_LD>(sn, L, pcol, pcol);
        // x = x+ + P+[:, 6:13] S^-1 (z - x+[6:13])
        if (kite && j == 0) {
            double y[7];
            for (int a = 0; a < 7; ++a) y[a] = z[(size_t)b * 7 + a] - xn[6 + a];
            ekf_state_update<NK, EKF_LD>(sn, L, xn, y, xn);
        }
    }
    if (col)
        for (int i = 0; i < NK; ++i) Pc[((size_t)b * NK + i) * NK + j] = pcol[i];
    if (kite && j == 0)
        for (int i = 0; i < NK; ++i) x[(size_t)b * NK + i] = xn[i];
