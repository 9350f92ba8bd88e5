"""Workload for timing the FULL prologue with and without an in-flight schedule
(DESIGN 4.16): B kites (default 4096), N = 20, delay = 0.1, delay_steps = 16,
one cold step and `steps` (default 20) warm steps through step_device.

    rocprofv3 --kernel-trace --stats -d out -- python tools/inflight_probe.py [B] [steps] [none|two] [dump.npy]

none: no schedule (k_prologue predicts under the previous u(t0), 16 substeps).
two:  every kite's line holds two pending commands that arrive 0.03 s and
      0.07 s into the window (three pieces: 5 + 7 + 5 substeps), refreshed
      before every step as FleetLoop(delay_comp="queue") does.
dump.npy (optional): u0 and the trajectory of the last step, for comparing two
builds of the library (KITE_NMPC_LIB) bit for bit.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import openkite_amd as ok  # noqa: E402
from bench import synthetic_x0  # noqa: E402
from openkite_amd import nmpc  # noqa: E402

N = 20


def main(B, steps, mode, dump):
    cfg = ok.default_config(N=N, delay=0.1, delay_steps=16)
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, B)
    try:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        f64 = dict(dtype=torch.float64, device="cuda")
        x0 = torch.from_numpy(synthetic_x0(B, 0, ctx)).cuda()
        u0, traj = torch.zeros((B, 4), **f64), torch.zeros((B, N + 1, 15), **f64)
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        line = torch.zeros((B, nmpc.DELAY_NLINE), **f64)
        t = 0.0
        for s in range(steps + 1):
            if mode == "two" and s > 0:
                line.zero_()
                line[:, nmpc.DELAY_COUNT] = 2.0
                line[:, nmpc.DELAY_U_FORCE:nmpc.DELAY_U_FORCE + 3] = u0[:, :3]
                line[:, nmpc.DELAY_T_ARR] = t + 0.03
                line[:, nmpc.DELAY_T_ARR + 1] = t + 0.07
                line[:, nmpc.DELAY_U:nmpc.DELAY_U + 3] = u0[:, :3]
                line[:, nmpc.DELAY_U + 4:nmpc.DELAY_U + 7] = u0[:, :3]
                ctx.set_inflight_device(line.data_ptr(), t)
            ctx.step_device(x0.data_ptr(), u0.data_ptr(), traj.data_ptr(), 0, 0, status.data_ptr())
            x0.copy_(traj[:, 1, :])
            t += cfg.dt
        torch.cuda.synchronize()
        if dump:
            np.save(dump, np.concatenate([u0.cpu().numpy().ravel(), traj.cpu().numpy().ravel()]))
        print(f"inflight_probe: B={B} steps={steps} mode={mode} finite={bool(torch.isfinite(traj).all())} "
              f"bad_inflight={int(((status & 128) != 0).sum())}")
    finally:
        ctx.use_own_stream()
        ctx.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 4096, int(a[1]) if len(a) > 1 else 20, a[2] if len(a) > 2 else "none",
         a[3] if len(a) > 3 else None)
