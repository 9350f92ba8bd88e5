"""Closed loop under three estimators: what the controller is handed, and what
an identification makes of the log.

    python tools/kin_ekf_closed_loop.py [B] [steps] [iters]

B kites (default 64) fly `steps` control periods (default 50) against GpuPlant
with +-10 % perturb_params rows and no wind, three times (iters: evaluations
of each identification, default the configuration's 12):
  ekf         FleetLoop(ekf=True): the aerodynamic filter with the creation model
  ekf+model   FleetLoop(ekf=True, estimator_model="controller") with one
              adaptation after steps / 2 periods (what FleetLoop(adapt=...) does
              when its log is full): the rows identified from the first half
              become the controller's, and so the filter's
  kin_ekf     FleetLoop(kin_ekf=True): the kinematic, model-free filter
For each it prints one JSON line: the RMS error of the estimate handed to the
controller against the plant's true state over the second half of the flight,
split into v_b, w_b, r, q, and the distance of the 21 coefficients identified
from the log of that half (starting from the nominal row) from the plant's:
RMS and median over kites and coefficients of |p_id - p_plant| / |p_nominal|,
next to the same distance of the nominal row itself.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import openkite_amd as ok  # noqa: E402
from bench import synthetic_x0  # noqa: E402
from openkite_amd.fleet import FleetLoop, FlightRecorder, GpuPlant, GpuStepper  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
HALF = STEPS // 2
ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 0
N = 20
IDX = [ok.ident_param_index(j) for j in range(ok.IDENT_NP)]


def fly(name, **kw):
    cfg = ok.default_config(N=N)
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, B)
    try:
        nominal = ctx.params.as_array()
        plant_rows = ok.perturb_params(ctx.params, B, 0.1, seed=77)
        ctx.plant_set_params(plant_rows)
        x0 = synthetic_x0(B, 0, ctx)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        plant = GpuPlant(ctx, cfg.dt / 2, 2, 4)
        icfg = ok.ident_default_config(h=cfg.dt, substeps=plant.steps * plant.substeps)
        if ITERS:
            icfg.iters = ITERS
        rec = FlightRecorder(B, HALF - 1, "cuda")
        adapt = kw.pop("adapt", False)
        loop = FleetLoop(GpuStepper(ctx), torch.from_numpy(x0).cuda(), N, cfg.dt, plant=plant, recorder=rec,
                         covariances=ok.ekf_default_covariances(), **kw)
        err, adapted = [], 0
        for k in range(STEPS):
            if k == HALF:
                if adapt:
                    out, _, _, status = rec.identify(ctx, icfg, nominal)
                    torch.cuda.synchronize()
                    st = status.cpu().numpy()
                    good = ((st & ok.IDENT_CONVERGED) != 0) & ((st & ok.IDENT_NAN) == 0)
                    ctx.set_params(np.where(good[:, None], out.cpu().numpy(), nominal[None]))
                    adapted = int(good.sum())
                rec.reset()                      # every run logs the second half
            truth = loop.xp.clone()
            loop.step()
            if k >= HALF:
                e = loop.xe - truth
                qs = loop.xe[:, 9:13] + truth[:, 9:13]          # q and -q are one attitude
                e[:, 9:13] = torch.where((qs.norm(dim=1) < e[:, 9:13].norm(dim=1))[:, None], qs, e[:, 9:13])
                err.append(e)
        torch.cuda.synchronize()
        assert rec.full, (rec.nx, rec.nu)
        e = torch.stack(err).cpu().numpy()
        rms = lambda a: float(np.sqrt(np.mean(a ** 2)))
        out, cost2, evals, status = rec.identify(ctx, icfg, nominal)
        torch.cuda.synchronize()
        rows = out.cpu().numpy()
        st = status.cpu().numpy()
        ok_fit = ((st & ok.IDENT_CONVERGED) != 0) & ((st & ok.IDENT_NAN) == 0)
        d = np.abs(rows[:, IDX] - plant_rows[:, IDX]) / np.abs(nominal[IDX])
        d0 = np.abs(nominal[IDX][None] - plant_rows[:, IDX]) / np.abs(nominal[IDX])
        print(json.dumps(dict(
            estimator=name, B=B, steps=STEPS, iters=int(icfg.iters), kites_adapted=adapted,
            rms_v=rms(e[:, :, 0:3]), rms_w=rms(e[:, :, 3:6]), rms_r=rms(e[:, :, 6:9]), rms_q=rms(e[:, :, 9:13]),
            fits_converged=int(ok_fit.sum()),
            ident_rms=rms(d[ok_fit]) if ok_fit.any() else None,
            ident_median=float(np.median(d[ok_fit])) if ok_fit.any() else None,
            ident_rms_all=rms(d), nominal_rms=rms(d0), nominal_median=float(np.median(d0)),
            rti_status_or=int(np.bitwise_or.reduce(loop.status.cpu().numpy())),
            plant_nan=int(loop.plant_status.cpu().numpy().any()))), flush=True)
    finally:
        ctx.use_own_stream()
        ctx.close()


fly("ekf", ekf=True)
fly("ekf+model", ekf=True, estimator_model="controller", adapt=True)
fly("kin_ekf", kin_ekf=True)
