"""The per-kite sensitivity kernel against the homogeneous one.

    python tools/perkite_probe.py [B] [reps]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/perkite_probe.py

At batch B (default 4096), for N = 20 and N = 40, it runs `reps` warm steps of a
context with the creation model (k_rk4_sens2<Dual2, double, false>: 8 kites x 8
direction pairs per wave) and of one with +-10 % per-kite rows
(k_rk4_sens2<Dual2, double, false, true>: one kite per wave, 8 intervals x 8
direction pairs, the 47 constants by scalar loads from the kite's table row;
with k_prologue_warm on warm steps and k_model_const once).  Under rocprofv3
the kernel durations come from the trace's statistics: compare the two
k_rk4_sens2 averages per horizon.  Expectation from lane counts: 24 / 20 = 1.2 x
at N = 20 (three waves per kite, half of the last idle), 1.0 x at N = 40.  The
script itself prints the rk4_sens phase of the step's own event timing.
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
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10

out = {"B": B, "reps": REPS}
for N in (20, 40):
    for name in ("homogeneous", "per_kite"):
        g = ok.BatchNMPC(ok.load_properties(), ok.default_config(N=N), B)
        try:
            g.set_stream(torch.cuda.current_stream().cuda_stream)
            if name == "per_kite":
                rows = torch.from_numpy(ok.perturb_params(g.params, B, 0.1, seed=1, fields=ok.IDENT_FIELDS)).cuda()
                g.set_params_device(rows.data_ptr(), B)
            x = torch.from_numpy(synthetic_x0(B, 0, g)).cuda()
            traj = torch.zeros((B, N + 1, 15), dtype=torch.float64, device="cuda")
            g.step_device(x.data_ptr(), 0, traj.data_ptr())      # cold
            x.copy_(traj[:, 1, :])
            g.step_device(x.data_ptr(), 0, traj.data_ptr())      # warm-up
            g.timing_start(REPS)
            for _ in range(REPS):
                x.copy_(traj[:, 1, :])
                g.step_device(x.data_ptr(), 0, traj.data_ptr())
            n, ms = g.timing_read()
            out[f"N{N}_{name}_rk4_sens_us"] = 1e3 * ms["rk4_sens"] / n
            out[f"N{N}_{name}_step_us"] = 1e3 * ms["total"] / n
            out[f"N{N}_{name}_nan"] = int(np.isnan(traj.cpu().numpy()).any())
        finally:
            g.close()
    out[f"N{N}_rk4_sens_ratio"] = out[f"N{N}_per_kite_rk4_sens_us"] / out[f"N{N}_homogeneous_rk4_sens_us"]
print(json.dumps(out))
