"""The identification's kernels at fleet size, beside k_rk4_sens2 of the headline step.

    python tools/ident_probe.py [--wind] [B] [T] [reps]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ident_probe.py [--wind]

At batch B (default 4096) it flies T = 100 samples of h = 0.02 per kite on the
plant simulator (per-kite aerodynamic coefficients +-10 %, sinusoidal thrust,
elevator and rudder), then runs, `reps` times, one identify_device with
iters = 8, substeps = 4, L = 1 from the nominal row, and a few RTI steps at
N = 20 so that k_rk4_sens2 is in the same trace.  Under rocprofv3 the kernel
durations come from the trace's statistics; per unit of work
  k_ident_accum:  average / (B T substeps 4 stages 21 directions)
  k_rk4_sens2:    average / (B N M 4 stages 16 tangents), N = 20, M = 2
The script itself prints stream-event times (launch overhead included), what
the fit reached, and the host time of the numpy reference (tests/ident_ref.py)
for one kite and one evaluation, for scale.

With --wind every kite's plant flies under its own constant wind (+-1.5 m/s per
axis, no gust), the wind log holds it in every row, and the identification is
the wind form (kite_nmpc_identify_wind_device: k_ident_accum_w in the trace).
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import openkite_amd as ok  # noqa: E402
from bench import synthetic_x0  # noqa: E402

WIND = "--wind" in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a != "--wind"]
B = int(ARGS[0]) if len(ARGS) > 0 else 4096
T = int(ARGS[1]) if len(ARGS) > 1 else 100
REPS = int(ARGS[2]) if len(ARGS) > 2 else 5
H, SUB, ITERS = 0.02, 4, 8

cfg = ok.default_config(N=20)
g = ok.BatchNMPC(ok.load_properties(), cfg, B)
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


# the logs: every kite's own plant under sinusoidal controls
truth = ok.perturb_params(kp, B, 0.1, 5, fields=ok.IDENT_FIELDS)
g.plant_set_params(truth)
Wd = None
if WIND:
    wind = np.random.default_rng(8).uniform(-1.5, 1.5, (B, 3))
    g.plant_set_wind(wind=wind)
    Wd = torch.from_numpy(np.ascontiguousarray(np.repeat(wind[:, None], T, axis=1))).cuda()          # (B, T, 3)
rng = np.random.default_rng(6)
ph = rng.uniform(0, 2 * np.pi, (B, 3))
t = np.arange(T) * H
Uh = np.stack([0.125 + 0.025 * np.sin(2 * np.pi * 3.0 * t[None] + ph[:, :1]),
               0.12 * np.sin(2 * np.pi * 7.0 * t[None] + ph[:, 1:2]),
               0.12 * np.sin(2 * np.pi * 5.0 * t[None] + ph[:, 2:3])], axis=2)          # (B, T, 3)
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

icfg = ok.ident_default_config(h=H, substeps=SUB, segment=1, iters=ITERS, lb_rel=0.5, ub_rel=0.5)
rows = torch.from_numpy(kp[None].copy()).cuda()
out = torch.zeros((B, 52), **dev)
cost2 = torch.zeros((B, 2), **dev)
evals = torch.zeros((B,), dtype=torch.int32, device="cuda")
status = torch.zeros((B,), dtype=torch.int32, device="cuda")
ws = torch.empty((ok.ident_workspace_doubles(icfg, B, T),), **dev)


def identify():
    g.identify_device(icfg, B, T, rows.data_ptr(), 1, X.data_ptr(), U.data_ptr(), out.data_ptr(), cost2.data_ptr(),
                      evals.data_ptr(), status.data_ptr(), ws.data_ptr(), wind=Wd.data_ptr() if WIND else 0)


res = {"B": B, "T": T, "substeps": SUB, "segment": 1, "iters": ITERS, "reps": REPS, "wind": WIND}
res["identify_device_us"] = timed(identify)
idx = [ok.ident_param_index(j) for j in range(ok.IDENT_NP)]
sc = np.where(kp[idx] != 0.0, np.abs(kp[idx]), 1.0)
err = np.abs((out.cpu().numpy()[:, idx] - truth[:, idx]) / sc).max(axis=1)
stt = status.cpu().numpy()
res["scaled_error_median"] = float(np.median(err))
res["scaled_error_max"] = float(err.max())
res["converged"] = int(((stt & ok.IDENT_CONVERGED) != 0).sum())
res["nan"] = int(((stt & ok.IDENT_NAN) != 0).sum())
res["evals_mean"] = float(evals.cpu().numpy().mean())
res["workspace_MB"] = ws.numel() * 8 / 1e6

# the headline step's kernels in the same session
x0 = torch.from_numpy(x_init).cuda()
u0 = torch.zeros((B, 4), **dev)
traj = torch.zeros((B, 21, 15), **dev)
diag = torch.zeros((B, 6), **dev)
rst = torch.zeros((B,), dtype=torch.int32, device="cuda")


def rti():
    g.step_device(x0.data_ptr(), u0.data_ptr(), traj.data_ptr(), 0, diag.data_ptr(), rst.data_ptr())


res["rti_step_us"] = timed(rti)

# the numpy reference, one kite and one evaluation (for scale; not a performance claim)
try:
    from tests import ident_ref as ref
    Xh, U0 = X[0].cpu().numpy(), Uh[0]
    t0 = time.perf_counter()
    if WIND:
        from tests import ident_wind_ref as wref
        wref.normal(kp, kp[ref.IDX], Xh, np.ascontiguousarray(U0), Wd[0].cpu().numpy(), icfg)
    else:
        ref.normal(kp, kp[ref.IDX], Xh, np.ascontiguousarray(U0), icfg)
    res["numpy_reference_one_kite_one_evaluation_s"] = time.perf_counter() - t0
except Exception as e:  # the oracle is test infrastructure: the probe runs without it
    res["numpy_reference_one_kite_one_evaluation_s"] = None
    res["numpy_reference_error"] = repr(e)
g.close()
print(json.dumps(res))
