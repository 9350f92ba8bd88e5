// rk4_sens2_body.inc -- one (kite b, interval k, direction pair d) of the
// sensitivity kernel: the body of k_rk4_sens2 (rti_kernels.hip), included by
// both of its lane mappings so that they execute the same arithmetic.  In
// scope: the template parameters DT, ST, WIND; P (ModelConst), b, k, d, N, M,
// h, X, U, AB, DEF, wind.
    const double* xk = X + ((size_t)b * (N + 1) + k) * NX;
    const double* uk = U + ((size_t)b * N + k) * NU;
    const int d0 = 2 * d, d1 = 2 * d + 1;
    const ST one = ST(1), zero = ST(0), hs = ST(h);
    DT x[NK], u[NKU];
#pragma unroll
    for (int i = 0; i < NK; ++i) x[i] = DT(ST(xk[i]), d0 == i ? one : zero, d1 == i ? one : zero);
#pragma unroll
    for (int j = 0; j < NKU; ++j) u[j] = DT(ST(uk[j]), d0 == NK + j ? one : zero, d1 == NK + j ? one : zero);
    // The RK4 stages are peeled at both ends: stage 0 evaluates the right-hand
    // side on x itself (no xs = x, acc = x copies), stage 3 forms no next-stage
    // state (nothing reads it).  The two middle stages stay one rolled loop.
    // Operands and their order are those of the four-stage loop: same bits.
    const ST w6 = hs / ST(6), w3 = hs / ST(3), hh = ST(0.5) * hs;
#pragma unroll 1
    for (int m = 0; m < M; ++m) {
        DT xs[NK], acc[NK], kv[NK];
        kite_rhs<DT, WIND>(P, x, u, kv, WIND ? wind + 3 * b : nullptr);
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            acc[i] = rk_axpy<DT, ST>(w6, kv[i], x[i]);
            xs[i] = rk_axpy<DT, ST>(hh, kv[i], x[i]);
        }
#pragma unroll 1
        for (int st = 1; st < 3; ++st) {
            kite_rhs<DT, WIND>(P, xs, u, kv, WIND ? wind + 3 * b : nullptr);
            const ST wn = (st < 2) ? hh : hs;
#pragma unroll
            for (int i = 0; i < NK; ++i) {
                acc[i] = rk_axpy<DT, ST>(w3, kv[i], acc[i]);
                xs[i] = rk_axpy<DT, ST>(wn, kv[i], x[i]);
            }
        }
        kite_rhs<DT, WIND>(P, xs, u, kv, WIND ? wind + 3 * b : nullptr);
#pragma unroll
        for (int i = 0; i < NK; ++i) x[i] = rk_axpy<DT, ST>(w6, kv[i], acc[i]);
    }
    double* ab = AB + ((size_t)b * N + k) * (NK * 16);
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        ab[i * 16 + d0] = (double)x[i].a;
        ab[i * 16 + d1] = (double)x[i].b;
    }
    if constexpr (std::is_same<ST, double>::value) {
        if (d == 0) {
            const double* xn = X + ((size_t)b * (N + 1) + k + 1) * NX;
            double* df = DEF + ((size_t)b * N + k) * NK;
#pragma unroll
            for (int i = 0; i < NK; ++i) df[i] = x[i].v - xn[i];
        }
    }
