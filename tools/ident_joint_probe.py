"""The joint identification's kernels at fleet size, beside the logged-wind ones.

    python tools/ident_joint_probe.py [--full] [B] [T] [reps]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ident_joint_probe.py --full

As tools/ident_probe.py --wind: at batch B (default 4096) it flies T = 100
samples of h = 0.02 per kite on the plant simulator (per-kite coefficients
+-10 %, a constant wind of +-1.5 m/s per axis, sinusoidal controls), substeps 4,
L = 1, start at the nominal row.

--full: `reps` single full evaluations (iters = 1: every kite is live) of the
logged-wind form (k_ident_accum_w, the true wind in the log) and of the joint
form (k_ident_accum_jw, no wind log), for the kernel trace: the two averages
are per full evaluation and from the same session.
Without it: one identify_joint_device with iters = 12 from w = 0, timed with
stream events, and what it reached; the logged-wind identification (iters = 12,
the true wind known) beside it.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import openkite_amd as ok  # noqa: E402
from bench import synthetic_x0  # noqa: E402

FULL = "--full" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a != "--full"]
B = int(ARGS[0]) if len(ARGS) > 0 else 4096
T = int(ARGS[1]) if len(ARGS) > 1 else 100
REPS = int(ARGS[2]) if len(ARGS) > 2 else 3
H, SUB = 0.02, 4
ITERS = 1 if FULL else 12

g = ok.BatchNMPC(ok.load_properties(), ok.default_config(N=20), B)
g.set_stream(torch.cuda.current_stream().cuda_stream)
kp = g.params.as_array()
x_init = synthetic_x0(B, 0, g)
dev = dict(dtype=torch.float64, device="cuda")


def timed(fn, reps=REPS):
    """Mean stream time [us] of fn over reps calls (one warm-up first)."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


truth = ok.perturb_params(kp, B, 0.1, 5, fields=ok.IDENT_FIELDS)
wind = np.random.default_rng(8).uniform(-1.5, 1.5, (B, 3))
g.plant_set_params(truth)
g.plant_set_wind(wind=wind)
Wd = torch.from_numpy(np.ascontiguousarray(np.repeat(wind[:, None], T, axis=1))).cuda()
rng = np.random.default_rng(6)
ph = rng.uniform(0, 2 * np.pi, (B, 3))
t = np.arange(T) * H
Uh = np.stack([0.125 + 0.025 * np.sin(2 * np.pi * 3.0 * t[None] + ph[:, :1]),
               0.12 * np.sin(2 * np.pi * 7.0 * t[None] + ph[:, 1:2]),
               0.12 * np.sin(2 * np.pi * 5.0 * t[None] + ph[:, 2:3])], axis=2)
U = torch.from_numpy(np.ascontiguousarray(Uh)).cuda()
X = torch.zeros((B, T + 1, 13), **dev)
xp = torch.from_numpy(x_init[:, :13].copy()).cuda()
u4 = torch.zeros((B, 4), **dev)
pst = torch.zeros((B,), dtype=torch.int32, device="cuda")
X[:, 0] = xp
for k in range(T):
    u4[:, :3] = U[:, k]
    g.plant_step_device(xp.data_ptr(), u4.data_ptr(), k * H, H, 1, SUB, pst.data_ptr())
    X[:, k + 1] = xp
torch.cuda.synchronize()

icfg = ok.ident_default_config(h=H, substeps=SUB, segment=1, iters=ITERS, lb_rel=0.5, ub_rel=0.5, lm0=1e-3)
wcfg = ok.ident_wind_default_config()
rows = torch.from_numpy(kp[None].copy()).cuda()
out = torch.zeros((B, 52), **dev)
wout = torch.zeros((B, 3), **dev)
cost2 = torch.zeros((B, 2), **dev)
evals = torch.zeros((B,), dtype=torch.int32, device="cuda")
status = torch.zeros((B,), dtype=torch.int32, device="cuda")
ws = torch.empty((ok.ident_joint_workspace_doubles(icfg, B, T),), **dev)      # serves both forms


def logged():
    g.identify_device(icfg, B, T, rows.data_ptr(), 1, X.data_ptr(), U.data_ptr(), out.data_ptr(), cost2.data_ptr(),
                      evals.data_ptr(), status.data_ptr(), ws.data_ptr(), wind=Wd.data_ptr())


def joint():
    g.identify_joint_device(icfg, wcfg, B, T, rows.data_ptr(), 1, X.data_ptr(), U.data_ptr(), out.data_ptr(),
                            wout.data_ptr(), cost2.data_ptr(), evals.data_ptr(), status.data_ptr(), ws.data_ptr())


idx = [ok.ident_param_index(j) for j in range(ok.IDENT_NP)]
sc = np.where(kp[idx] != 0.0, np.abs(kp[idx]), 1.0)


def reached(prefix, res, with_wind):
    err = np.abs((out.cpu().numpy()[:, idx] - truth[:, idx]) / sc).max(axis=1)
    stt = status.cpu().numpy()
    res[prefix + "scaled_error_median"] = float(np.median(err))
    res[prefix + "scaled_error_max"] = float(err.max())
    res[prefix + "converged"] = int(((stt & ok.IDENT_CONVERGED) != 0).sum())
    res[prefix + "nan"] = int(((stt & ok.IDENT_NAN) != 0).sum())
    res[prefix + "evals_mean"] = float(evals.cpu().numpy().mean())
    if with_wind:
        ew = np.abs(wout.cpu().numpy() - wind).max(axis=1)
        res[prefix + "wind_error_median"] = float(np.median(ew))
        res[prefix + "wind_error_max"] = float(ew.max())
        res[prefix + "wind_at_bound"] = int(((stt & ok.IDENT_WIND_AT_BOUND) != 0).sum())


res = {"B": B, "T": T, "substeps": SUB, "segment": 1, "iters": ITERS, "reps": REPS, "full": FULL}
res["identify_wind_device_us"] = timed(logged)
reached("logged_", res, False)
res["identify_joint_device_us"] = timed(joint)
reached("joint_", res, True)
res["joint_workspace_MB"] = ws.numel() * 8 / 1e6
res["logged_workspace_MB"] = ok.ident_workspace_doubles(icfg, B, T) * 8 / 1e6
g.close()
print(json.dumps(res))
