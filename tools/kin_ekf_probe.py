"""k_ekf_kin at a production batch, for a kernel trace.

    python tools/kin_ekf_probe.py [B] [reps]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/kin_ekf_probe.py

At batch B (default 4096), dt = 0.05, substeps 5, with the update and the
reference node's frame, it launches one warm-up and `reps` timed times (default
11: 12 launches in a trace), every launch from the same x, P.  Under rocprofv3
the kernel durations come from the trace; the script prints the stream-event
time per launch (the restoring copies of x and P included) and whether any
estimate went non-finite.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import openkite_amd as ok  # noqa: E402
from bench import synthetic_x0  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 11
DT, SUB = 0.05, 5

g = ok.BatchNMPC(ok.load_properties(), ok.default_config(N=20), B)
try:
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    x0 = torch.from_numpy(synthetic_x0(B, 0, g)[:, :13].copy()).cuda()
    z = x0[:, 6:13].contiguous()
    W, V, P0 = (torch.from_numpy(a).cuda() for a in ok.ekf_default_covariances())
    P_0 = P0[None].repeat(B, 1, 1).contiguous()
    x, P = x0.clone(), P_0.clone()
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    fr = ok.pose_frame_default()

    def call():
        x.copy_(x0); P.copy_(P_0)
        g.kin_ekf_step_device(B, DT, SUB, x.data_ptr(), P.data_ptr(), z.data_ptr(), W.data_ptr(), V.data_ptr(),
                              st.data_ptr(), frame=fr)

    call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        call()
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"B": B, "reps": REPS, "dt": DT, "substeps": SUB, "kin_ekf_call_us": 1e3 * e0.elapsed_time(e1) / REPS,
                      "status_bits": int(st.max().item()),
                      "nonfinite": int((~torch.isfinite(x)).sum().item() + (~torch.isfinite(P)).sum().item())}))
finally:
    g.use_own_stream()
    g.close()
