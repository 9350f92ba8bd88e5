"""Does the adaptation chain make a fleet fly better?  The closed-loop score of
the same kites with and without it.

    python tools/score_study.py [B] [episodes] [episode_steps]      the study
    python tools/score_study.py --cost [B] [episodes]               the scorer's launch cost

The study.  B kites (default 256) fly GpuPlant with +-10 % perturb_params rows
against the nominal controller, in `episodes` (default 12) episodes of
`episode_steps` (default 40) control periods with FleetLoop.restart() between
them, as bench.py --episode does (an unbroken loop loses kites from step ~45,
DESIGN 6).  Every loop flies the same kites from the same launch states, with
an EpisodeScore on the stream; the log of the adapting loops holds 24 periods,
so each episode identifies once, at its period 24, and the models carry over
to the next episode.

  none         no adaptation
  adapt        recorder + adapt: the 21 coefficients identified per kite become
               the controller's models
  adapt+ekf    the same, flown through the aerodynamic EKF, which filters with
               the controller's models (ekf=True, estimator_model="controller")
  wind/none    no adaptation, under a 1.5 m/s plant wind the controller is not told
  wind/joint   recorder + adapt + ident_wind="joint" under the same wind: the
               wind is identified with the 21 and handed to the controller

One JSON line per loop: the fleet summary over all episodes (EpisodeScore.summary:
the raw 16 and the derived figures), and "tail": the same figures over the
episodes after the first, when every kite that adapted flies its own model
from the launch (sums only: differences of the raw summaries).

--cost.  A headline loop (no plant, B default 4096) with and without a scorer,
alternating episodes of 40 steps timed with device events; prints the median
step time of both and their ratio.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import openkite_amd as ok  # noqa: E402
from bench import synthetic_x0  # noqa: E402
from openkite_amd.fleet import EpisodeScore, FleetLoop, FlightRecorder, GpuPlant, GpuStepper  # noqa: E402

N = 20
LOG_T = 24
WIND = 1.5


def tail_of(raw_all, raw_first, dt):
    """The derived figures over the episodes after the first (sum slots only)."""
    d = np.asarray(raw_all) - np.asarray(raw_first)
    d[ok.SCORE_KITES] = raw_all[ok.SCORE_KITES]
    out = ok.score_derive(d, dt)
    for k in ("max_d", "min_speed", "ever_lost", "kites_lost_fraction"):     # not differences
        out.pop(k)
    return out


def fly(name, B, episodes, steps, wind=False, **kw):
    cfg = ok.default_config(N=N)
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, B)
    try:
        ctx.plant_set_params(ok.perturb_params(ctx.params, B, 0.1, seed=77))
        if wind:
            d = np.random.default_rng(78).normal(size=(B, 3))
            ctx.plant_set_wind(wind=WIND * d / np.linalg.norm(d, axis=1, keepdims=True))
        x0 = synthetic_x0(B, 0, ctx)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        plant = GpuPlant(ctx, cfg.dt / 2, 2, 4)
        adapt = kw.pop("adapt", None)
        if adapt == "plain":
            kw.update(recorder=FlightRecorder(B, LOG_T, "cuda"),
                      adapt=ok.ident_default_config(h=cfg.dt, substeps=plant.steps * plant.substeps))
        elif adapt == "joint":
            # the settings of the joint identification's closed-loop test: a kite whose
            # fit has not converged when the evaluations run out keeps its row
            kw.update(recorder=FlightRecorder(B, LOG_T, "cuda"), ident_wind="joint",
                      adapt=ok.ident_default_config(h=cfg.dt, substeps=plant.steps * plant.substeps, lb_rel=0.5,
                                                    ub_rel=0.5, lm0=1e-3, iters=32))
        if kw.get("ekf"):
            kw["covariances"] = ok.ekf_default_covariances()
        score = EpisodeScore(B, device="cuda")
        loop = FleetLoop(GpuStepper(ctx), torch.from_numpy(x0).cuda(), N, cfg.dt, plant=plant, scorer=score, **kw)
        first, adapted = None, []
        for e in range(episodes):
            if e:
                loop.restart()
            for _ in range(steps):                      # nothing here waits for the device
                loop.step()
            if adapt:
                st = loop.ident_status
                adapted.append(int((((st & ok.IDENT_CONVERGED) != 0) & ((st & ok.IDENT_NAN) == 0)).sum().item()))
            if e == 0:
                first = score.summary()["raw"]
        s = score.summary()
        out = dict(loop=name, B=B, episodes=episodes, episode_steps=steps, plant_wind=WIND if wind else 0.0,
                   adaptations=getattr(loop, "adapt_count", 0), fits_converged_per_episode=adapted, **s)
        if episodes > 1:
            out["tail"] = tail_of(s["raw"], first, cfg.dt)
        print(json.dumps(out), flush=True)
        return out
    finally:
        ctx.use_own_stream()
        ctx.close()


def table(rows):
    cols = [("rms_d", "rms d [m]"), ("max_d", "max d [m]"), ("mean_track", "mean l_track"), ("mean_u", "mean l_u"),
            ("mean_rate", "mean rate"), ("mean_speed", "mean |v| [m/s]"), ("min_speed", "min |v|"),
            ("lost_fraction", "lost periods"), ("kites_lost_fraction", "kites ever lost"), ("lap_rate", "laps/s")]
    print("| loop | " + " | ".join(h for _, h in cols) + " | tail rms d | tail mean l_track | tail lost |")
    print("|---|" + "---|" * (len(cols) + 3))
    for r in rows:
        t = r.get("tail", {})
        print(f"| {r['loop']} | " + " | ".join(f"{r[k]:.4g}" for k, _ in cols)
              + f" | {t.get('rms_d', float('nan')):.4g} | {t.get('mean_track', float('nan')):.4g}"
              + f" | {t.get('lost_fraction', float('nan')):.4g} |")


def study(B, episodes, steps):
    rows = [fly("none", B, episodes, steps),
            fly("adapt", B, episodes, steps, adapt="plain"),
            fly("adapt+ekf", B, episodes, steps, adapt="plain", ekf=True, estimator_model="controller"),
            fly("wind/none", B, episodes, steps, wind=True),
            fly("wind/joint", B, episodes, steps, wind=True, adapt="joint")]
    table(rows)


def cost(B, episodes, steps=40):
    cfg = ok.default_config(N=N)
    ctxs = [ok.BatchNMPC(ok.load_properties(), cfg, B) for _ in range(2)]
    try:
        loops = []
        for i, ctx in enumerate(ctxs):
            x0 = synthetic_x0(B, 0, ctx)
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            loops.append(FleetLoop(GpuStepper(ctx), torch.from_numpy(x0).cuda(), N, cfg.dt,
                                   scorer=EpisodeScore(B, device="cuda") if i else None))
        ms = [[], []]
        for e in range(episodes + 1):                   # episode 0 warms up
            for i, loop in enumerate(loops):
                loop.restart()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(steps):
                    loop.step()
                b.record()
                b.synchronize()
                if e:
                    ms[i].append(a.elapsed_time(b) / steps)
        plain, scored = float(np.median(ms[0])), float(np.median(ms[1]))
        s = loops[1].scorer.summary()
        print(json.dumps(dict(cost=True, B=B, episodes=episodes, episode_steps=steps, step_ms_plain=plain,
                              step_ms_scored=scored, ratio=scored / plain, step_ms_plain_all=ms[0],
                              step_ms_scored_all=ms[1], rms_d=s["rms_d"], lost_fraction=s["lost_fraction"])),
              flush=True)
    finally:
        for ctx in ctxs:
            ctx.use_own_stream()
            ctx.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--cost":
        cost(int(args[1]) if len(args) > 1 else 4096, int(args[2]) if len(args) > 2 else 8)
    else:
        study(int(args[0]) if args else 256, int(args[1]) if len(args) > 1 else 12,
              int(args[2]) if len(args) > 2 else 40)
