"""Float64 reference of the closed-loop scorer (score_kernels.hip): the global
closest point on the path (64 samples of theta with the lowest-index arg-min,
then the safeguarded Newton iteration clamped to the sample's neighbours), the
lost rule, every accumulator slot of a kite's row, the memory row, and the
fleet summary (math.fsum).  One kite per call, written in scalar Python from
the same equations as the kernel.

One switch (``mp=True``) evaluates the per-period quantities -- theta*, d, d^2,
l_track, l_u, the rate, the speed and the progress step -- in mpmath at 50
digits from the same float64 inputs: the distance between the two is the
reference's own rounding error, the envelope the GPU bars are built from
(tests/test_score_ref.py measures it, tests/test_score.py uses it).

The inputs of the GPU tests are generated here (``positions``,
``episode_inputs``, ``lap_inputs``), so the envelope is measured over exactly
what the kernels are given.  Checked by tests/test_score_ref.py."""
import math

import numpy as np

NACC, NSUM, NMEM = 16, 16, 8
(N, N_LOST, EVER_LOST, SUM_D2, MAX_D, SUM_TRACK, SUM_U, SUM_RATE, SUM_SPEED, MIN_SPEED, PROGRESS, N_MIN_SPEED,
 N_QP_NOT_CONV, N_STATE_BOUND, N_RATE, SPARE) = range(16)
KITES = 15
MEM_THETA, MEM_U, MEM_VALID = 0, 1, 5
ST_NAN, ST_QP_NOT_CONV, ST_MIN_SPEED, ST_STATE_BOUND, ST_THETA_WRAP, ST_STEP_REJECTED, ST_RESTART = 1, 2, 4, 8, 16, 32, 64
PLANT_NAN = 1
LOSING = ST_NAN | ST_STEP_REJECTED | ST_RESTART
SAMPLES, NEWTON = 64, 12
INT_SLOTS = (N, N_LOST, EVER_LOST, N_MIN_SPEED, N_QP_NOT_CONV, N_STATE_BOUND, N_RATE, SPARE)

# ---- the rounding envelope ---------------------------------------------------
# Worst |float64 reference - 50-digit value| of each per-period quantity over
# the inputs of tests/test_score.py (``envelope_inputs``), measured on the CPU
# by tests/test_score_ref.py::test_rounding_envelope, which prints the measured
# figures and holds each recorded one within [measured, 1.25 measured].  The GPU
# bar of a quantity is BAR_FACTOR times its envelope: the margin for an equally
# valid operation order, fma contraction, and OCML's sincos against libm.
ENVELOPE = {
    "theta": 4.4e-16,     # rad            (measured 4.341e-16)
    "d": 1.2e-15,         # m              (1.197e-15)
    "d2": 8.8e-16,        # m^2            (8.714e-16)
    "track": 1.2e-12,     # controller units: Q (Sx e)^2 reaches 1e3 at 1.5 m   (1.172e-12)
    "u": 4.4e-17,         #                (4.316e-17)
    "rate": 2.0e-15,      #                (1.971e-15)
    "speed": 1.1e-15,     # m/s            (1.001e-15)
    "dtheta": 9.3e-16,    # rad, one progress step   (9.288e-16)
}
BAR_FACTOR = 32.0


def bar(q):
    return BAR_FACTOR * ENVELOPE[q]


# ---- arithmetic back ends ----------------------------------------------------
class _F64:
    pi = math.pi
    two_pi = 6.283185307179586
    sin, cos, sqrt = staticmethod(math.sin), staticmethod(math.cos), staticmethod(math.sqrt)
    newton = NEWTON

    @staticmethod
    def num(x):
        return float(x)


_MP_CACHE = []


def _mp_backend():
    if not _MP_CACHE:
        _MP_CACHE.append(_make_mp_backend())
    return _MP_CACHE[0]


def _make_mp_backend():
    import mpmath
    ctx = mpmath.mp.clone()
    ctx.dps = 50

    class _MP:
        pi = ctx.pi + 0
        two_pi = 2 * ctx.pi
        sin, cos, sqrt = staticmethod(ctx.sin), staticmethod(ctx.cos), staticmethod(ctx.sqrt)
        newton = 60                         # to the 50-digit fixed point

        @staticmethod
        def num(x):
            return ctx.mpf(float(x))
    return _MP


# ---- constants of a configuration ---------------------------------------------
def consts(cfg):
    """What the scorer takes from an ``NmpcConfig``: the path, Q, R, Sx[6:9], Su."""
    return dict(K=int(cfg.path_harmonics), R=float(cfg.path_radius), alt=float(cfg.path_altitude),
                F=np.array(list(cfg.path_fourier), dtype=np.float64).reshape(3, 17), q=[float(v) for v in cfg.path_q],
                Q=[float(v) for v in cfg.Q], Sr=[float(cfg.Sx[6 + a]) for a in range(3)],
                Rw=[float(v) for v in cfg.R], Su=[float(v) for v in cfg.Su])


def _rot(C, v, M):
    """q^-1 (x) [0, v] (x) q with q = (w, u): (w^2 - u.u) v + 2 (u.v) u - 2 w (u x v)."""
    w, ux, uy, uz = (M.num(t) for t in C["q"])
    ww_uu = w * w - (ux * ux + uy * uy + uz * uz)
    uv2 = 2 * (ux * v[0] + uy * v[1] + uz * v[2])
    cx, cy, cz = uy * v[2] - uz * v[1], uz * v[0] - ux * v[2], ux * v[1] - uy * v[0]
    w2 = 2 * w
    return [ww_uu * v[0] + uv2 * ux - w2 * cx, ww_uu * v[1] + uv2 * uy - w2 * cy, ww_uu * v[2] + uv2 * uz - w2 * cz]


def path(C, th, M=_F64):
    """P, P', P'' at theta (the rotated curve), harmonics by the angle-addition recurrence."""
    c, s = M.cos(th), M.sin(th)
    K = C["K"]
    if K == 0:
        R, alt = M.num(C["R"]), M.num(C["alt"])
        p, dp, ddp = [R * c, R * s, alt], [-R * s, R * c, M.num(0)], [-R * c, -R * s, M.num(0)]
    else:
        F = C["F"]
        p = [M.num(F[a, 0]) for a in range(3)]
        dp = [M.num(0)] * 3
        ddp = [M.num(0)] * 3
        ck, sk = c, s
        for k in range(1, K + 1):
            for a in range(3):
                ak, bk = M.num(F[a, 2 * k - 1]), M.num(F[a, 2 * k])
                p[a] = p[a] + (ak * ck + bk * sk)
                dp[a] = dp[a] + k * (bk * ck - ak * sk)
                ddp[a] = ddp[a] - (k * k) * (ak * ck + bk * sk)
            ck, sk = ck * c - sk * s, sk * c + ck * s
    return _rot(C, p, M), _rot(C, dp, M), _rot(C, ddp, M)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def nearest_sample(C, r):
    """The lowest-index nearest of the 64 samples (float64)."""
    best, jmin = None, SAMPLES
    for j in range(SAMPLES):
        P, _, _ = path(C, j * (_F64.two_pi / SAMPLES))
        e = [P[a] - r[a] for a in range(3)]
        d2 = _dot(e, e)
        if best is None or d2 < best:
            best, jmin = d2, j
    return jmin


def closest_point(C, r, mp=False):
    """(theta*, d, E = P(theta*) - r) of the global closest point; NaN for a
    non-finite r.  mp: the Newton iteration and the distance at 50 digits, from
    the float64 arithmetic's nearest sample."""
    r = [float(v) for v in r]
    if not all(math.isfinite(v) for v in r):
        return math.nan, math.nan, [math.nan] * 3
    M = _mp_backend() if mp else _F64
    jmin = nearest_sample(C, r)
    step = M.two_pi / SAMPLES
    th = jmin * step
    lo, hi = th - step, th + step
    rr = [M.num(v) for v in r]
    for _ in range(M.newton):
        P, dP, ddP = path(C, th, M)
        e = [P[a] - rr[a] for a in range(3)]
        g, gn = _dot(e, dP), _dot(dP, dP)
        h = gn + _dot(e, ddP)
        if h <= 0:
            h = gn
        if not h > 0:
            break
        tn = th - g / h
        tn = lo if tn < lo else (hi if tn > hi else tn)
        if tn == th:
            break
        th = tn
    P, _, _ = path(C, th, M)
    E = [P[a] - rr[a] for a in range(3)]
    return th, M.sqrt(_dot(E, E)), E


def wrap(x, M=_F64):
    """To (-pi, pi], for |x| < 3 pi."""
    if x > M.pi:
        return x - M.two_pi
    if x <= -M.pi:
        return x + M.two_pi
    return x


def period(C, x13, u4, mem, first, mp=False):
    """The per-period quantities of one finite (x13, u4): theta, d, d2, track,
    u, speed, and with a valid predecessor rate and dtheta (else None)."""
    M = _mp_backend() if mp else _F64
    th, d, E = closest_point(C, x13[6:9], mp)
    e = [M.num(C["Sr"][a]) * E[a] for a in range(3)]
    track = (M.num(C["Q"][0]) * (e[0] * e[0]) + M.num(C["Q"][1]) * (e[1] * e[1])) + M.num(C["Q"][2]) * (e[2] * e[2])
    s = [M.num(C["Su"][i]) * M.num(u4[i]) for i in range(4)]
    lu = ((M.num(C["Rw"][0]) * (s[0] * s[0]) + M.num(C["Rw"][1]) * (s[1] * s[1])) + M.num(C["Rw"][2]) * (s[2] * s[2])
          ) + M.num(C["Rw"][3]) * (s[3] * s[3])
    v = [M.num(x13[i]) for i in range(3)]
    speed = M.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    out = dict(theta=th, d=d, d2=d * d, track=track, u=lu, speed=speed, rate=None, dtheta=None)
    if not first and mem[MEM_VALID] != 0.0:
        rr = [M.num(C["Su"][i]) * (M.num(u4[i]) - M.num(mem[MEM_U + i])) for i in range(4)]
        out["rate"] = ((rr[0] * rr[0] + rr[1] * rr[1]) + rr[2] * rr[2]) + rr[3] * rr[3]
        # the predecessor's theta* is a float64 datum (what mem holds)
        out["dtheta"] = wrap(th - M.num(mem[MEM_THETA]), M)
    return out


def is_lost(x13, u4, status, plant_status):
    return bool((plant_status & PLANT_NAN) or (status & LOSING) or not np.all(np.isfinite(x13))
                or not np.all(np.isfinite(u4)))


def score_step(C, x13, u4, status, plant_status, first, acc, mem):
    """One control period of one kite: acc (16,) and mem (8,) updated in place."""
    status = 0 if status is None else int(status)
    plant_status = 0 if plant_status is None else int(plant_status)
    lost = is_lost(x13, u4, status, plant_status)
    if not lost:
        q = period(C, x13, u4, mem, first)
        lost = not all(math.isfinite(q[k]) for k in ("d2", "track", "u", "speed"))
    if lost:
        acc[N_LOST] += 1.0
        acc[EVER_LOST] = 1.0
        mem[MEM_VALID] = 0.0
        return
    n = acc[N]
    acc[N] = n + 1.0
    acc[SUM_D2] += q["d2"]
    acc[MAX_D] = q["d"] if n == 0.0 else max(acc[MAX_D], q["d"])
    acc[SUM_TRACK] += q["track"]
    acc[SUM_U] += q["u"]
    acc[SUM_SPEED] += q["speed"]
    acc[MIN_SPEED] = q["speed"] if n == 0.0 else min(acc[MIN_SPEED], q["speed"])
    if q["rate"] is not None:
        acc[SUM_RATE] += q["rate"]
        acc[PROGRESS] += q["dtheta"]
        acc[N_RATE] += 1.0
    if status & ST_MIN_SPEED:
        acc[N_MIN_SPEED] += 1.0
    if status & ST_QP_NOT_CONV:
        acc[N_QP_NOT_CONV] += 1.0
    if status & ST_STATE_BOUND:
        acc[N_STATE_BOUND] += 1.0
    mem[MEM_THETA] = q["theta"]
    mem[MEM_U:MEM_U + 4] = u4
    mem[MEM_VALID] = 1.0


def score_batch(C, x13, u4, status, plant_status, first, acc, mem):
    """score_step for every kite of a batch (rows of acc / mem in place)."""
    for b in range(x13.shape[0]):
        score_step(C, x13[b], u4[b], None if status is None else status[b],
                   None if plant_status is None else plant_status[b], first, acc[b], mem[b])


def summary(acc):
    """The raw fleet summary (16,) of acc (B, 16) with exact sums (math.fsum)."""
    acc = np.asarray(acc, dtype=np.float64).reshape(-1, NACC)
    out = np.zeros(NSUM)
    for k in range(NACC):
        out[k] = math.fsum(acc[:, k])
    scored = acc[acc[:, N] > 0]
    out[MAX_D] = scored[:, MAX_D].max() if len(scored) else 0.0
    out[MIN_SPEED] = scored[:, MIN_SPEED].min() if len(scored) else 0.0
    out[KITES] = float(acc.shape[0])
    return out


# ---- vectorised path (direct cos k theta, independent of the recurrence) ------
def path_np(C, th):
    """P, P', P'' (3, n) at the angles th (n,)."""
    th = np.asarray(th, dtype=np.float64)
    if C["K"] == 0:
        F = np.zeros((3, 17)); F[0, 1] = C["R"]; F[1, 2] = C["R"]; F[2, 0] = C["alt"]
        K = 1
    else:
        F, K = C["F"], C["K"]
    p = np.stack([np.full_like(th, F[a, 0]) for a in range(3)])
    d = np.zeros_like(p); dd = np.zeros_like(p)
    for k in range(1, K + 1):
        c, s = np.cos(k * th), np.sin(k * th)
        for a in range(3):
            ak, bk = F[a, 2 * k - 1], F[a, 2 * k]
            p[a] += ak * c + bk * s; d[a] += k * (bk * c - ak * s); dd[a] += -k * k * (ak * c + bk * s)
    w, u = C["q"][0], np.array(C["q"][1:])

    def rot(v):
        return (w * w - u @ u) * v + 2.0 * np.outer(u, u @ v) - 2.0 * w * np.cross(u, v, axis=0)
    return rot(p), rot(d), rot(dd)


def unrotate(C, v):
    """The inverse of the path's rotation (q (x) [0, v] (x) q^-1)."""
    w, u = C["q"][0], np.array(C["q"][1:])
    v = np.asarray(v, dtype=np.float64)
    return (w * w - u @ u) * v + 2.0 * (u @ v) * u + 2.0 * w * np.cross(u, v)


def local_minima(C, r, n=4096):
    """Sorted distances of the local minima of ||P(theta) - r|| (grid of n, Newton refined)."""
    r = np.asarray(r, dtype=np.float64)
    ths = 2.0 * np.pi * np.arange(n) / n
    P, _, _ = path_np(C, ths)
    d2 = ((P - r[:, None]) ** 2).sum(0)
    out = []
    for i in np.nonzero((d2 <= np.roll(d2, 1)) & (d2 < np.roll(d2, -1)))[0]:
        th = ths[i]
        for _ in range(30):
            P1, dP, ddP = (a[:, 0] for a in path_np(C, [th]))
            e = P1 - r
            h = dP @ dP + e @ ddP
            if h <= 0:
                break
            th -= (e @ dP) / h
        P1 = path_np(C, [th])[0][:, 0]
        out.append(float(np.linalg.norm(P1 - r)))
    return sorted(out)


def condition_ok(C, r):
    """The input condition of the scorer's tests: within 1.5 m of the path, at
    least 0.5 m from the circle's axis, and the best two local minima of the
    distance at least 1e-3 m apart."""
    m = local_minima(C, r)
    ru = unrotate(C, r)
    return bool(m and m[0] <= 1.5 and math.hypot(ru[0], ru[1]) >= 0.5 and (len(m) < 2 or m[1] - m[0] >= 1e-3))


def brute_force(C, r):
    """(theta, d): 200 000 samples, then an unclamped Newton refinement."""
    r = np.asarray(r, dtype=np.float64)
    ths = np.linspace(0.0, 2.0 * np.pi, 200001)[:-1]
    P, _, _ = path_np(C, ths)
    th = ths[int(np.argmin(((P - r[:, None]) ** 2).sum(0)))]
    for _ in range(50):
        P1, dP, ddP = (a[:, 0] for a in path_np(C, [th]))
        e = P1 - r
        h = dP @ dP + e @ ddP
        if h <= 0:
            break
        th -= (e @ dP) / h
    P1 = path_np(C, [th])[0][:, 0]
    return float(th), float(np.linalg.norm(P1 - r))


# ---- the inputs of the GPU tests ------------------------------------------------
def positions(C, n, seed):
    """n positions (n, 3) that meet ``condition_ok``: a point of the path plus an
    offset of up to 1.5 m in a random direction; every tenth (0, 10, ...) sits
    exactly on the path."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        t = rng.uniform(0.0, 2.0 * np.pi)
        off = rng.normal(size=3)
        off *= rng.uniform(0.0, 1.5) / np.linalg.norm(off)
        if len(out) % 10 == 0:
            off *= 0.0
        r = np.array(path(C, t)[0]) + off
        if condition_ok(C, r):
            out.append(r)
    return np.array(out)


def episode_inputs(C, B, T, seed):
    """T periods of B kites: x13 (T, B, 13), u4 (T, B, 4), status and
    plant_status (T, B) int32.  The positions meet ``condition_ok``; the status
    words mix the counted bits, and a few periods carry a losing bit."""
    rng = np.random.default_rng(seed)
    pos = positions(C, T * B, seed + 1).reshape(T, B, 3)
    x = np.zeros((T, B, 13))
    x[..., 0:3] = rng.normal(size=(T, B, 3)) * np.array([1.5, 0.5, 0.5]) + np.array([5.0, 0.0, 0.0])
    x[..., 3:6] = rng.normal(size=(T, B, 3))
    x[..., 6:9] = pos
    q = rng.normal(size=(T, B, 4))
    x[..., 9:13] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    u = np.stack([rng.uniform(0.0, 0.3, (T, B)), rng.uniform(-0.3, 0.3, (T, B)), rng.uniform(-0.3, 0.3, (T, B)),
                  rng.uniform(-5.0, 5.0, (T, B))], axis=-1)
    st = np.zeros((T, B), dtype=np.int32)
    for bit in (ST_QP_NOT_CONV, ST_MIN_SPEED, ST_STATE_BOUND, ST_THETA_WRAP):
        st |= np.where(rng.uniform(size=(T, B)) < 0.35, bit, 0).astype(np.int32)
    ps = np.zeros((T, B), dtype=np.int32)
    if T >= 4:
        st[2, 0] |= ST_STEP_REJECTED                # kite 0 loses period 2
        if B > 1:
            ps[T - 3, B - 1] = PLANT_NAN            # the last kite is frozen for one period
    return x, u, st, ps


# the closest-point test: 22 positions per path, a slice per batch shape
CP_SEED = {"circle": 11, "fourier": 12}
CP_SLICES = {9: (0, 9), 5: (9, 14), 4: (14, 18), 3: (18, 21), 1: (21, 22)}
# the scoring tests: one episode of 9 kites x 6 periods per path; a smaller batch is its first kites
EP_B, EP_T = 9, 6
EP_SEED = {"circle": 21, "fourier": 22}


def gpu_test_positions(Cs):
    """(name, C, positions) of everything tests/test_score.py hands to the kernels;
    Cs: {"circle": consts, "fourier": consts}."""
    for kind, C in Cs.items():
        yield f"cp/{kind}", C, positions(C, 22, CP_SEED[kind])
        yield f"episode/{kind}", C, episode_inputs(C, EP_B, EP_T, EP_SEED[kind])[0][..., 6:9].reshape(-1, 3)
    for direction in (1, -1):
        yield f"lap/{direction}", Cs["circle"], lap_inputs(Cs["circle"], direction)[0][:, 6:9]


def gpu_test_periods(Cs):
    """(C, x13, u4, mem, first) of every scored period of those tests, mem as the
    float64 reference carries it."""
    for kind, C in Cs.items():
        for r in positions(C, 22, CP_SEED[kind]):
            x = np.zeros(13); x[6:9] = r
            yield C, x, np.zeros(4), np.zeros(NMEM), True
        x, u, st, ps = episode_inputs(C, EP_B, EP_T, EP_SEED[kind])
        acc, mem = np.zeros((EP_B, NACC)), np.zeros((EP_B, NMEM))
        for t in range(EP_T):
            for b in range(EP_B):
                if not is_lost(x[t, b], u[t, b], int(st[t, b]), int(ps[t, b])):
                    yield C, x[t, b], u[t, b], mem[b].copy(), t == 0
            score_batch(C, x[t], u[t], st[t], ps[t], t == 0, acc, mem)
    for direction in (1, -1):
        C = Cs["circle"]
        x, u = lap_inputs(C, direction)
        acc, mem = np.zeros(NACC), np.zeros(NMEM)
        for k in range(13):
            yield C, x[k], u[k], mem.copy(), k == 0
            score_step(C, x[k], u[k], 0, 0, k == 0, acc, mem)


def lap_inputs(C, direction=1, start_deg=200.0):
    """A kite stepped 12 x 30 degrees round the path from start_deg (13 periods,
    crossing 2 pi), exactly on it: x13 (13, 13), u4 (13, 4)."""
    x = np.zeros((13, 13)); u = np.zeros((13, 4))
    for k in range(13):
        th = math.radians(start_deg + direction * 30.0 * k)
        x[k, 6:9] = path(C, th)[0]
        x[k, 0:3] = [4.0 + 0.125 * k, 0.25, -0.5]
        x[k, 9] = 1.0
        u[k] = [0.1 + 0.01 * k, 0.02 * k - 0.1, 0.1 - 0.015 * k, 0.3 * k - 2.0]
    return x, u
