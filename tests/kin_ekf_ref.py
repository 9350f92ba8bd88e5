"""numpy float64 reference of the kinematic (pose-only) EKF: the model
RigidBodyKinematics (kite.cpp:622-661), the filter KiteEKF(Function, Function)
(kiteEKF.cpp:54-126) with the kernel's semantics (k_ekf_kin), the node's
two-pose initialisation (ekf_node.cpp:68-132) and its pose frame
(optitrack2world, :148-169).  Written from the equations with quaternion
product matrices, independently of the kernel's scalar closed forms; checked
by tests/test_kin_ekf_ref.py, used as the reference by tests/test_kin_ekf.py.

One kite per call; x13 = (v_b, w_b, r, q), q = (w, x, y, z)."""
import numpy as np

LAMBDA = -10.0
EKF_NAN, EKF_S_NOT_PD, EKF_INIT_BAD = 1, 2, 4

# the node's frame (ekf_node.cpp: brf_offset, brf_rotation, the +2.77 of :166)
DEFAULT_FRAME = dict(offset=(-0.09, 0.0, -0.02), rotation=(0.0, -1.0, 0.0, 0.0), shift=(0.0, 0.0, 2.77))
IDENTITY_FRAME = dict(offset=(0.0, 0.0, 0.0), rotation=(1.0, 0.0, 0.0, 0.0), shift=(0.0, 0.0, 0.0))


def qleft(p):
    """L(p) with p (x) q = L(p) q."""
    w, x, y, z = p
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])


def qright(q):
    """R(q) with p (x) q = R(q) p."""
    w, x, y, z = q
    return np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])


def qmul(p, q):
    return qleft(p) @ np.asarray(q)


def conj(q):
    q = np.asarray(q)
    return np.concatenate([q[:1], -q[1:]])


def rotate(q, v):
    """vec( q (x) [0, v] (x) conj(q) ), q not normalised."""
    return qmul(qmul(q, np.concatenate([[0.0], v])), conj(q))[1:]


def f(x):
    """The model's right-hand side; complex x allowed (no conjugation anywhere)."""
    x = np.asarray(x)
    v, w, q = x[0:3], x[3:6], x[9:13]
    out = np.zeros(13, dtype=x.dtype)
    out[6:9] = rotate(q, v)
    out[9:13] = 0.5 * qmul(q, np.concatenate([[0.0], w])) + 0.5 * LAMBDA * q * (np.sum(q * q) - 1.0)
    return out


def jac(x):
    """Analytic df/dx (13 x 13) from the product matrices:
    r' = E L(q) R(conj q) [0; v], q' = 1/2 L(q) [0; w] + stabiliser."""
    x = np.asarray(x, dtype=np.float64)
    v, w, q = x[0:3], x[3:6], x[9:13]
    E = np.eye(4)[1:]                       # vec()
    C = np.diag([1.0, -1.0, -1.0, -1.0])    # conj
    v4 = np.concatenate([[0.0], v]); w4 = np.concatenate([[0.0], w])
    J = np.zeros((13, 13))
    # d r'/d v: the rotation matrix E L(q) R(conj q) E'
    J[6:9, 0:3] = E @ qleft(q) @ qright(conj(q)) @ E.T
    # d r'/d q: q appears on the left, and conjugated on the right
    J[6:9, 9:13] = E @ (qright(conj(q)) @ qright(v4) + qleft(q) @ qleft(v4) @ C)
    J[9:13, 3:6] = 0.5 * qleft(q) @ E.T
    J[9:13, 9:13] = 0.5 * qright(w4) + 0.5 * LAMBDA * ((q @ q - 1.0) * np.eye(4) + 2.0 * np.outer(q, q))
    return J


def rk4(x, h):
    x = np.asarray(x, dtype=np.float64)
    k1 = f(x); k2 = f(x + 0.5 * h * k1); k3 = f(x + 0.5 * h * k2); k4 = f(x + h * k3)
    return x + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def frame(z, fr):
    """The frame change of one pose z7 = (r, q); fr None: z as given."""
    z = np.asarray(z, dtype=np.float64)
    if fr is None:
        return z.copy()
    off, rot, sh = (np.asarray(fr[k], dtype=np.float64) for k in ("offset", "rotation", "shift"))
    r, q = z[:3], z[3:]
    r = r + rotate(q, off)
    r = rotate(rot, r) + sh
    q = qmul(qmul(rot, q), conj(rot))
    return np.concatenate([r, q])


def step(x, P, dt, substeps, z, W, V, fr=None, order="AP_first"):
    """One call of the filter for one kite: (x, P, status).  order: the two
    association orders of A P A' (the spread between them is the rounding a
    different summation order can cause)."""
    x0 = np.asarray(x, dtype=np.float64).copy(); P0 = np.asarray(P, dtype=np.float64).copy()
    if not (np.all(np.isfinite(x0)) and np.all(np.isfinite(P0))):
        return x0, P0, EKF_NAN
    x, P = x0.copy(), P0.copy()
    if z is not None:
        z = frame(z, fr)
        if z[3:] @ x[9:13] < 0.0:
            z[3:] = -z[3:]
    h = dt / substeps
    status = 0
    for _ in range(substeps):
        A = np.eye(13) + jac(x) * h
        xn = rk4(x, h)
        Pn = (A @ P) @ A.T + W if order == "AP_first" else A @ (P @ A.T) + W
        if not (np.all(np.isfinite(xn)) and np.all(np.isfinite(Pn))):
            return x, P, EKF_NAN                    # the last finite estimate
        x, P = xn, Pn
    if z is None:
        return x, P, status
    S = P[6:, 6:] + V
    try:
        Lc = np.linalg.cholesky(np.tril(S) + np.tril(S, -1).T)     # from the lower triangle
        pd = bool(np.all(np.isfinite(Lc))) and bool(np.all(np.isfinite(z)))
    except np.linalg.LinAlgError:
        pd = False
    if not pd:
        return x, P, EKF_S_NOT_PD
    Sl = np.tril(S) + np.tril(S, -1).T
    K = np.linalg.solve(Sl, P[:, 6:].T).T           # P[:, 6:13] S^-1
    xu = x + K @ (z - x[6:])
    Pu = P - K @ P[6:, :]
    if not (np.all(np.isfinite(xu)) and np.all(np.isfinite(Pu))):
        return x, P, EKF_NAN
    return xu, 0.5 * (Pu + Pu.T), status


def init(prev, new, dt, fr=None):
    """(x13, status) from two poses dt apart; status EKF_INIT_BAD: no x13 (None)."""
    mp, mn = frame(prev, fr), frame(new, fr)
    if not (np.isfinite(dt) and dt > 0.0 and np.all(np.isfinite(mp)) and np.all(np.isfinite(mn))):
        return None, EKF_INIT_BAD
    rdot = (mn[:3] - mp[:3]) / dt
    qp = mp[3:]
    vb = qmul(qmul(conj(qp), np.concatenate([[0.0], rdot])), qp)[1:]
    qn = -mn[3:] if qp @ mn[3:] < 0.0 else mn[3:]
    dq = qmul(conj(qp), qn)
    wb = (2.0 / dt) * (dq - np.array([1.0, 0.0, 0.0, 0.0]))[1:]
    return np.concatenate([vb, wb, mn]), 0
