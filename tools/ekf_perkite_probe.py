"""The per-kite EKF kernels against the homogeneous ones.

    python tools/ekf_perkite_probe.py [B] [reps]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ekf_perkite_probe.py

At batch B (default 4096), dt = 0.05, it launches one warm-up and `reps` timed
times (default 11: 12 launches in a trace) each
  * k_ekf and k_ekf_wind (substeps 5) of a context whose estimators keep the
    creation model (the homogeneous kernels, the model a kernel argument), and
  * k_ekf_pk and k_ekf_wind_pk of a context with +-10 % per-kite rows in the
    controller and the estimators on them (kite_nmpc_set_estimator_model):
    each kite's row copied to LDS from the controller's table,
every launch from the same x, P, with the update.  Under rocprofv3 the kernel
durations come from the trace's statistics; the script itself prints
stream-event times per launch (the restoring copies of x and P included, and
measured on their own) and whether any estimate went non-finite.
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
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 11
DT, SUB = 0.05, 5
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


out = {"B": B, "reps": REPS, "dt": DT, "substeps": SUB}
for name in ("homogeneous", "per_kite"):
    g = ok.BatchNMPC(ok.load_properties(), ok.default_config(N=20), B)
    try:
        g.set_stream(torch.cuda.current_stream().cuda_stream)
        if name == "per_kite":
            rows = torch.from_numpy(ok.perturb_params(g.params, B, 0.1, seed=1, fields=ok.IDENT_FIELDS)).cuda()
            g.set_params_device(rows.data_ptr(), B)
            g.set_estimator_model(ok.EST_MODEL_CONTROLLER)
        x_init = synthetic_x0(B, 0, g)
        rng = np.random.default_rng(1)
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
        W13, _, P13 = (torch.from_numpy(a).cuda() for a in ok.ekf_default_covariances())
        x13_0 = x16_0[:, :13].contiguous()
        P13_0 = P13[None].repeat(B, 1, 1).contiguous()
        x13, Pk = x13_0.clone(), P13_0.clone()

        def wind_call():
            x16.copy_(x16_0); Pw.copy_(P16_0)
            g.wind_ekf_step_device(B, DT, SUB, x16.data_ptr(), u3.data_ptr(), Pw.data_ptr(), z.data_ptr(),
                                   W16.data_ptr(), V.data_ptr(), st.data_ptr())

        def ekf_call():
            x13.copy_(x13_0); Pk.copy_(P13_0)
            g.ekf_step_device(B, DT / SUB, x13.data_ptr(), u3.data_ptr(), Pk.data_ptr(), z.data_ptr(), W13.data_ptr(),
                              V.data_ptr())

        def wind_copies():
            x16.copy_(x16_0); Pw.copy_(P16_0)

        def ekf_copies():
            x13.copy_(x13_0); Pk.copy_(P13_0)

        out[f"{name}_wind_copies_us"] = timed(wind_copies)
        out[f"{name}_wind_ekf_call_us"] = timed(wind_call)
        out[f"{name}_ekf_copies_us"] = timed(ekf_copies)
        out[f"{name}_ekf_call_us"] = timed(ekf_call)
        out[f"{name}_wind_ekf_status_bits"] = int(st.max().item())
        out[f"{name}_nonfinite"] = int((~torch.isfinite(x16)).sum().item() + (~torch.isfinite(x13)).sum().item()
                                       + (~torch.isfinite(Pw)).sum().item() + (~torch.isfinite(Pk)).sum().item())
    finally:
        g.use_own_stream()
        g.close()
print(json.dumps(out))
