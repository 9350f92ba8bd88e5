"""k_plant_delay against k_plant, variant by variant.

    python tools/plant_delay_probe.py [B] [reps]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/plant_delay_probe.py

At batch B (default 4096) and the shape of tools/plant_kernel_probe.py (3 plant
steps of 0.02 s, 4 RK4 substeps each) it runs, `reps` times each and for each of
the six <PERKITE, WIND> variants, plant_step_device (k_plant) and
plant_step_delayed_device (k_plant_delay) with a command sent every period and
a latency of 0.03 s, so that every launch appends to the line, pops from it at
the period's third tick and compacts it.  Under rocprofv3 the kernel durations
come from the trace's statistics: compare k_plant_delay<P, W> with k_plant<P, W>.
The script itself prints stream-event times (launch overhead included) and
their ratios.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import openkite_amd as ok  # noqa: E402
from bench import synthetic_x0  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
H, STEPS, SUB, TAU = 0.02, 3, 4, 0.03

g = ok.BatchNMPC(ok.load_properties(), ok.default_config(N=20), B)
g.set_stream(torch.cuda.current_stream().cuda_stream)
x_init = synthetic_x0(B, 0, g)
rng = np.random.default_rng(1)
P = ok.perturb_params(g.params, B, 0.1, seed=1)
W0 = rng.uniform(-0.3, 0.3, (B, 3))
A = rng.uniform(-0.2, 0.2, (B, 3))
hz, ph = rng.uniform(0.5, 2.0, B), rng.uniform(-3.0, 3.0, B)
f64 = dict(dtype=torch.float64, device="cuda")
u4 = torch.zeros((B, 4), **f64)
u4[:, 0] = 0.12
tau = torch.full((B,), TAU, **f64)
ua = torch.zeros((B, 4), **f64)
st = torch.zeros((B,), dtype=torch.int32, device="cuda")


def timed(fn):
    """Mean stream time [us] of fn(k) over REPS calls k = 1 .. REPS (call 0 warms up)."""
    fn(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(1, REPS + 1):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / REPS


def plain():
    x = torch.from_numpy(x_init[:, :13].copy()).cuda()
    return lambda k: g.plant_step_device(x.data_ptr(), u4.data_ptr(), k * STEPS * H, H, STEPS, SUB, st.data_ptr())


def delayed():
    x = torch.from_numpy(x_init[:, :13].copy()).cuda()
    line = torch.zeros((B, ok.DELAY_NLINE), **f64)
    return lambda k: g.plant_step_delayed_device(x.data_ptr(), u4.data_ptr(), tau.data_ptr(), line.data_ptr(),
                                                 k * STEPS * H, H, STEPS, SUB, ua.data_ptr(), st.data_ptr())


out = {"B": B, "reps": REPS, "steps": STEPS, "substeps": SUB, "tau": TAU}
for pk in (False, True):
    for wm, wind in ((0, None), (1, (W0,)), (2, (W0, A, hz, ph))):
        g.plant_set_params(P if pk else None)
        g.plant_set_wind(*(wind or ()))
        a, b = timed(plain()), timed(delayed())
        key = f"{'per_kite' if pk else 'shared'}_{('calm', 'wind', 'gust')[wm]}"
        out[key] = {"k_plant_us": a, "k_plant_delay_us": b, "ratio": b / a}
out["dropped"] = int(((st & ok.PLANT_CMD_DROPPED) != 0).sum().item())
g.close()
print(json.dumps(out))
