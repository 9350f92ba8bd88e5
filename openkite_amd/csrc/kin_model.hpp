// kin_model.hpp -- rigid-body kinematics, the model of the pose-only filter.
//
// RigidBodyKinematics (src/kite_model/kite.cpp:622-661), the model the
// reference's estimator node hands to KiteEKF(Function, Function)
// (ekf_node.cpp:235-241): no control, no parameters.
//
//   x13 = [v_b(3) w_b(3) r(3) q(4)],  q = (w, u)
//   v_b' = 0,  w_b' = 0                                      (random walks)
//   r'   = vec( q (x) [0, v_b] (x) conj(q) )                 (conj, not a normalised
//                                                             inverse: kitemath.cpp:25-29)
//   q'   = 1/2 q (x) [0, w_b] + 1/2 lambda q (q.q - 1),  lambda = -10
//          (kite.cpp:639-640; the kite model's stabiliser has lambda = -5)
//
// The Jacobian df/dx is written in closed form.  Rows 0..5 are zero; the other
// seven rows hold four dense blocks, 49 structural non-zeros of 169:
//
//   d r'/d v_b (3 x 3) = (w^2 - u.u) I + 2 u u' + 2 w [u]x
//   d r'/d q   (3 x 4) = [ 2 w v + 2 u x v | -2 v u' + 2 (u.v) I + 2 u v' - 2 w [v]x ]
//   d q'/d w_b (4 x 3) = 1/2 [ -u' ; w I + [u]x ]
//   d q'/d q   (4 x 4) = 1/2 [ 0  -w_b' ; w_b  -[w_b]x ] + 1/2 lambda ((q.q - 1) I + 2 q q')
//
// with [a]x the cross-product matrix, [a]x b = a x b.  kite_rhs (kite_model.hpp)
// is not reused with another lambda: its kernels keep their instruction streams.
#pragma once
#include <hip/hip_runtime.h>

namespace kite {

constexpr double kKinLambda = -10.0;   // kite.cpp:639

// the four blocks of df/dx
struct KinJac {
    double rv[3][3];   // d r'/d v_b
    double rq[3][4];   // d r'/d q
    double qw[4][3];   // d q'/d w_b
    double qq[4][4];   // d q'/d q
};

// f[13] = f(x13)
__host__ __device__ __forceinline__ void kin_rhs(const double* x, double* f) {
    const double v0 = x[0], v1 = x[1], v2 = x[2];
    const double o0 = x[3], o1 = x[4], o2 = x[5];
    const double w = x[9], a = x[10], b = x[11], c = x[12];
    for (int i = 0; i < 6; ++i) f[i] = 0.0;
    // (w^2 - u.u) v + 2 (u.v) u + 2 w (u x v)
    const double uu = a * a + b * b + c * c;
    const double s = w * w - uu;
    const double uv2 = 2.0 * (a * v0 + b * v1 + c * v2);
    const double w2 = 2.0 * w;
    f[6] = s * v0 + uv2 * a + w2 * (b * v2 - c * v1);
    f[7] = s * v1 + uv2 * b + w2 * (c * v0 - a * v2);
    f[8] = s * v2 + uv2 * c + w2 * (a * v1 - b * v0);
    // 1/2 (-u.w_b, w w_b + u x w_b) + 1/2 lambda (q.q - 1) q
    const double lam = (0.5 * kKinLambda) * ((w * w + uu) - 1.0);
    f[9] = -0.5 * (a * o0 + b * o1 + c * o2) + lam * w;
    f[10] = 0.5 * (w * o0 + (b * o2 - c * o1)) + lam * a;
    f[11] = 0.5 * (w * o1 + (c * o0 - a * o2)) + lam * b;
    f[12] = 0.5 * (w * o2 + (a * o1 - b * o0)) + lam * c;
}

// the blocks of df/dx at x13
__host__ __device__ __forceinline__ void kin_jac(const double* x, KinJac& J) {
    const double v[3] = {x[0], x[1], x[2]};
    const double o[3] = {x[3], x[4], x[5]};
    const double w = x[9];
    const double u[3] = {x[10], x[11], x[12]};
    const double uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    const double s = w * w - uu;
    const double uv = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
    const double w2 = 2.0 * w;
    // [u]x and [v]x, [w_b]x by their entries: cr(a, i, k) = ([a]x)_{ik}
    auto cr = [](const double* a, int i, int k) -> double {
        if (i == k) return 0.0;
        const int m = 3 - i - k;                       // the third index
        return ((k - i + 3) % 3 == 1) ? -a[m] : a[m];  // (0,1): -a2, (1,2): -a0, (2,0): -a1
    };
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k)
            J.rv[i][k] = (i == k ? s : 0.0) + 2.0 * u[i] * u[k] + w2 * cr(u, i, k);
    const double uxv[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    for (int i = 0; i < 3; ++i) {
        J.rq[i][0] = w2 * v[i] + 2.0 * uxv[i];
        for (int k = 0; k < 3; ++k)
            J.rq[i][1 + k] = 2.0 * (u[i] * v[k] - v[i] * u[k]) + (i == k ? 2.0 * uv : 0.0) - w2 * cr(v, i, k);
    }
    for (int k = 0; k < 3; ++k) J.qw[0][k] = -0.5 * u[k];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) J.qw[1 + i][k] = 0.5 * ((i == k ? w : 0.0) + cr(u, i, k));
    const double q[4] = {w, u[0], u[1], u[2]};
    const double dn = 0.5 * kKinLambda * ((w * w + uu) - 1.0);    // 1/2 lambda (q.q - 1)
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k) {
            double p;                                              // the product's part
            if (i == 0) p = (k == 0) ? 0.0 : -0.5 * o[k - 1];
            else if (k == 0) p = 0.5 * o[i - 1];
            else p = -0.5 * cr(o, i - 1, k - 1);
            J.qq[i][k] = p + (i == k ? dn : 0.0) + kKinLambda * q[i] * q[k];
        }
}

// ---- quaternion helpers of the pose frame and the initialisation ------------
// vec( q (x) [0, v] (x) conj(q) ), q = (w, u) not normalised
__host__ __device__ __forceinline__ void kin_rot(const double* q, const double* v, double* o) {
    const double w = q[0], a = q[1], b = q[2], c = q[3];
    const double s = w * w - (a * a + b * b + c * c);
    const double uv2 = 2.0 * (a * v[0] + b * v[1] + c * v[2]);
    const double w2 = 2.0 * w;
    const double o0 = s * v[0] + uv2 * a + w2 * (b * v[2] - c * v[1]);
    const double o1 = s * v[1] + uv2 * b + w2 * (c * v[0] - a * v[2]);
    const double o2 = s * v[2] + uv2 * c + w2 * (a * v[1] - b * v[0]);
    o[0] = o0; o[1] = o1; o[2] = o2;
}
// p (x) q (kitemath.cpp quat_multiply); o may alias neither
__host__ __device__ __forceinline__ void kin_qmul(const double* p, const double* q, double* o) {
    o[0] = p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3];
    o[1] = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2];
    o[2] = p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1];
    o[3] = p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0];
}

// The motion-capture -> world change of a pose (optitrack2world,
// ekf_node.cpp:148-169); the fields of kite_pose_frame (kite_nmpc.h)
struct PoseFrame {
    double offset[3], rotation[4], shift[3];
};
// z7 = (r, q) in place:
//   r <- r + vec(q (x) [0, offset] (x) conj(q))
//   r <- vec(rot (x) [0, r] (x) conj(rot)) + shift,  q <- rot (x) q (x) conj(rot)
__host__ __device__ __forceinline__ void kin_frame(const PoseFrame& F, double* z) {
    double ob[3], r[3], t[4], qo[4];
    kin_rot(z + 3, F.offset, ob);
    for (int i = 0; i < 3; ++i) r[i] = z[i] + ob[i];
    kin_rot(F.rotation, r, ob);
    for (int i = 0; i < 3; ++i) z[i] = ob[i] + F.shift[i];
    const double rc[4] = {F.rotation[0], -F.rotation[1], -F.rotation[2], -F.rotation[3]};
    kin_qmul(F.rotation, z + 3, t);
    kin_qmul(t, rc, qo);
    for (int i = 0; i < 4; ++i) z[3 + i] = qo[i];
}

}  // namespace kite
