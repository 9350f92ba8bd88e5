"""k_plant against the k_predict launches it replaces, and the plant's share of a fleet step.

    python tools/plant_kernel_probe.py [B] [reps]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/plant_kernel_probe.py

At batch B (default 4096) it runs, `reps` times each:
  * plant_step_device(steps=3, substeps=4) with the nominal plant (k_plant<false, 0>),
    with per-kite parameters (k_plant<true, 0>), with per-kite parameters and a
    constant wind (<true, 1>) and a gust (<true, 2>), and the gust alone (<false, 2>);
  * the same nominal work the way the driver did it before: three
    kite_nmpc_predict(tf = 0.02, steps = 4) calls (three k_predict launches).
Under rocprofv3 the kernel durations come from the trace's statistics: compare
k_plant<false, 0> with three times k_predict's average.  The script itself
prints stream-event times (launch overhead included) and the share of one
FleetLoop step (N = 20, device-resident, gust plant) the plant phase takes.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import openkite_amd as ok  # noqa: E402
from openkite_amd.fleet import FleetLoop, GpuPlant, GpuStepper  # noqa: E402
from bench import synthetic_x0  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
H, STEPS, SUB = 0.02, 3, 4

cfg = ok.default_config(N=20)
g = ok.BatchNMPC(ok.load_properties(), cfg, B)
g.set_stream(torch.cuda.current_stream().cuda_stream)
x_init = synthetic_x0(B, 0, g)
rng = np.random.default_rng(1)
P = ok.perturb_params(g.params, B, 0.1, seed=1)
W0 = rng.uniform(-0.3, 0.3, (B, 3))
A = rng.uniform(-0.2, 0.2, (B, 3))
hz, ph = rng.uniform(0.5, 2.0, B), rng.uniform(-3.0, 3.0, B)
x13 = torch.from_numpy(x_init[:, :13].copy()).cuda()
u4 = torch.zeros((B, 4), dtype=torch.float64, device="cuda")
u4[:, 0] = 0.12
st = torch.zeros((B,), dtype=torch.int32, device="cuda")


def timed(fn):
    """Mean stream time [us] of fn over REPS calls (one warm-up first)."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / REPS


def plant_call():
    x = x13.clone()
    return lambda: g.plant_step_device(x.data_ptr(), u4.data_ptr(), 0.0, H, STEPS, SUB, st.data_ptr())


out = {"B": B, "reps": REPS}
variants = [("nominal", None, None), ("per_kite", P, None), ("per_kite_wind", P, (W0,)),
            ("per_kite_gust", P, (W0, A, hz, ph)), ("gust", None, (W0, A, hz, ph))]
for name, params, wind in variants:
    g.plant_set_params(params)
    g.plant_set_wind(*(wind or ()))
    out[f"plant_{name}_us"] = timed(plant_call())
g.plant_set_params(None)
g.plant_set_wind(None)

# the parent's way: one kite_nmpc_predict per plant step (host pointers: the
# event time includes the copies, the kernel time is in the trace)
x15 = np.zeros((B, 15))
x15[:, :13] = x_init[:, :13]
u4h = u4.cpu().numpy()


def predict3():
    x = x15
    for _ in range(STEPS):
        x = g.predict(x, u4h, H, SUB)


out["predict_x3_host_call_us"] = timed(predict3)

# share of a closed-loop step: device-resident FleetLoop with the gust plant
g.plant_set_params(P)
g.plant_set_wind(W0, A, hz, ph)
plant = GpuPlant(g, cfg.dt / 2, 2, 5)
loop = FleetLoop(GpuStepper(g), torch.from_numpy(x_init).cuda(), 20, cfg.dt, plant=plant)
loop.step()
out["fleet_step_us"] = timed(loop.step)
xp = loop.xp.clone()
out["fleet_plant_phase_us"] = timed(lambda: plant.advance(xp, loop.u0, 0.0, loop.plant_status))
out["plant_share_of_step"] = out["fleet_plant_phase_us"] / out["fleet_step_us"]
out["plant_nan"] = int(loop.plant_status.sum().item())
g.close()
print(json.dumps(out))
