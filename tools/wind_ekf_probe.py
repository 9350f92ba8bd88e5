"""k_ekf_wind against the five k_ekf launches of an estimator phase, and the estimator's share of a fleet step.

    python tools/wind_ekf_probe.py [B] [reps]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/wind_ekf_probe.py

At batch B (default 4096), dt = 0.05 and 5 substeps it runs, `reps` times each:
  * one wind_ekf_step_device(dt, substeps = 5, z): one k_ekf_wind launch;
  * what FleetLoop(ekf=True) issues per control period: five ekf_step_device
    calls of dt / 5, the last with z (five k_ekf launches).
Under rocprofv3 the kernel durations come from the trace's statistics: compare
k_ekf_wind's average with five times k_ekf's.  The script itself prints
stream-event times (launch overhead included) and the share of one FleetLoop
step (N = 20, device-resident, plant with a constant wind) that the estimator
phase -- k_ekf_wind and the wind hand-over to the controller -- takes.
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
DT, SUB = 0.05, 5

cfg = ok.default_config(N=20)
g = ok.BatchNMPC(ok.load_properties(), cfg, B)
g.set_stream(torch.cuda.current_stream().cuda_stream)
x_init = synthetic_x0(B, 0, g)
rng = np.random.default_rng(1)
dev = dict(dtype=torch.float64, device="cuda")


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


u3 = torch.zeros((B, 3), **dev)
u3[:, 0] = 0.12
z = torch.from_numpy(x_init[:, 6:13].copy()).cuda()
st = torch.zeros((B,), dtype=torch.int32, device="cuda")

W16, V, P16 = (torch.from_numpy(a).cuda() for a in ok.wind_ekf_default_covariances())
x16_0 = torch.zeros((B, 16), **dev)
x16_0[:, :13] = torch.from_numpy(x_init[:, :13].copy()).cuda()
x16_0[:, 13:] = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 3))).cuda()
P16_0 = P16[None].repeat(B, 1, 1).contiguous()
x16, Pw = x16_0.clone(), P16_0.clone()


def wind_call():
    x16.copy_(x16_0); Pw.copy_(P16_0)
    g.wind_ekf_step_device(B, DT, SUB, x16.data_ptr(), u3.data_ptr(), Pw.data_ptr(), z.data_ptr(), W16.data_ptr(),
                           V.data_ptr(), st.data_ptr())


W13, _, P13 = (torch.from_numpy(a).cuda() for a in ok.ekf_default_covariances())
x13_0 = x16_0[:, :13].contiguous()
P13_0 = P13[None].repeat(B, 1, 1).contiguous()
x13, Pk = x13_0.clone(), P13_0.clone()


def ekf5_call():
    x13.copy_(x13_0); Pk.copy_(P13_0)
    for j in range(SUB):
        g.ekf_step_device(B, DT / SUB, x13.data_ptr(), u3.data_ptr(), Pk.data_ptr(), z.data_ptr() if j == SUB - 1 else 0,
                          W13.data_ptr(), V.data_ptr())


def copies_only():
    x16.copy_(x16_0); Pw.copy_(P16_0)


out = {"B": B, "reps": REPS, "dt": DT, "substeps": SUB}
out["copies_us"] = timed(copies_only)
out["wind_ekf_call_us"] = timed(wind_call)
out["ekf_x5_call_us"] = timed(ekf5_call)
out["wind_ekf_nan"] = int((st & ok.EKF_NAN).sum().item())

# share of a closed-loop step: device-resident FleetLoop with a plant wind
g.plant_set_wind(rng.uniform(-0.5, 0.5, (B, 3)))
plant = GpuPlant(g, cfg.dt / 2, 2, 5)
loop = FleetLoop(GpuStepper(g), torch.from_numpy(x_init).cuda(), 20, cfg.dt, wind_ekf=True,
                 covariances=ok.wind_ekf_default_covariances(), plant=plant)
loop.step()
loop.step()
out["fleet_step_us"] = timed(loop.step)
xe, Pe = loop.xe.clone(), loop.P.clone()
stepper = loop.stepper


def estimator_phase():
    stepper.wind_ekf(cfg.dt, loop.ekf_substeps, xe, loop.u3, Pe, loop.z, loop.W, loop.V, st)
    stepper.set_wind_device(xe[:, 13:], loop.wind_max)


out["fleet_estimator_phase_us"] = timed(estimator_phase)
out["estimator_share_of_step"] = out["fleet_estimator_phase_us"] / out["fleet_step_us"]
out["fleet_ekf_nan"] = int((loop.ekf_status & ok.EKF_NAN).sum().item())
out["fleet_plant_nan"] = int(loop.plant_status.sum().item())
g.close()
print(json.dumps(out))
