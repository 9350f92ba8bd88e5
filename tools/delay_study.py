"""Does the controller's delay compensation help against the delay it assumes?
The closed-loop score of the same kites behind a command line.

    python tools/delay_study.py [B] [episodes] [episode_steps]

B kites (default 256) fly the nominal GpuPlant (the controller's own model, no
wind) in `episodes` (default 12) episodes of `episode_steps` (default 40)
control periods with FleetLoop.restart() between them, as tools/score_study.py
does.  Every row flies the same kites from the same launch states with the same
seeds, scored with an EpisodeScore on the stream.  A row is a pair: the plant's
actuation delay (fleet.ActuationDelay: mean +- deviation, seconds; None: the
undelayed plant) and config.delay, the delay the controller compensates
(k_prologue predicts the measured state that far under the previous control):

  0 / 0               no delay anywhere
  0 / 0.1             what nmpf_driver flies by default: a compensation without a delay
  0.1 / 0             the node's delay, uncompensated
  0.1 / 0.1           the node: delay and compensation
  0.1+-0.005 / 0.1    the same with the injector's jitter
  0.02+-0.005 / 0     the injector's own defaults (transport_delay.cpp: 20 +- 5 ms)
  0.05 / 0            one control period, the largest constant latency the line sustains
  0.05 / 0.05         the same, compensated

The line charges every accepted command its own latency after the one before it
(the node's sleep per message), so a constant latency above the control period
(0.1 s here) is a channel that falls behind until it is full; from then on the
oldest command is dropped before its turn comes and nothing arrives any more.
The 0.1 rows fly that, the 0.05 rows a pure one-period delay.

One JSON line per row (EpisodeScore.summary plus "cmd_dropped", the commands
the full lines dropped, and "cmds", the commands sent), then the table.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import openkite_amd as ok  # noqa: E402
from bench import synthetic_x0  # noqa: E402
from openkite_amd.fleet import ActuationDelay, EpisodeScore, FleetLoop, GpuPlant, GpuStepper  # noqa: E402

N = 20
ROWS = [("0 / 0", None, 0.0, 0.0), ("0 / 0.1", None, 0.0, 0.1), ("0.1 / 0", 0.1, 0.0, 0.0), ("0.1 / 0.1", 0.1, 0.0, 0.1),
        ("0.1+-0.005 / 0.1", 0.1, 0.005, 0.1), ("0.02+-0.005 / 0", 0.02, 0.005, 0.0),
        ("0.05 / 0", 0.05, 0.0, 0.0), ("0.05 / 0.05", 0.05, 0.0, 0.05)]


def fly(name, B, episodes, steps, mean, deviation, comp):
    cfg = ok.default_config(N=N, delay=comp, delay_steps=16)
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, B)
    try:
        x0 = synthetic_x0(B, 0, ctx)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        delay = ActuationDelay(B, mean, deviation, seed=81, device="cuda") if mean is not None else None
        plant = GpuPlant(ctx, cfg.dt / 2, 2, 4, delay=delay)
        score = EpisodeScore(B, device="cuda")
        loop = FleetLoop(GpuStepper(ctx), torch.from_numpy(x0).cuda(), N, cfg.dt, plant=plant, scorer=score)
        dropped = torch.zeros((), dtype=torch.int64, device="cuda")
        for e in range(episodes):
            if e:
                loop.restart()
            for _ in range(steps):                      # nothing here waits for the device
                loop.step()
                dropped += ((loop.plant_status & ok.PLANT_CMD_DROPPED) != 0).sum()
        s = score.summary()
        out = dict(row=name, B=B, episodes=episodes, episode_steps=steps, plant_delay=mean, plant_delay_dev=deviation,
                   config_delay=comp, cmd_dropped=int(dropped.item()), cmds=B * episodes * steps, **s)
        print(json.dumps(out), flush=True)
        return out
    finally:
        ctx.use_own_stream()
        ctx.close()


def table(rows):
    print("| plant delay / config.delay [s] | rms d [m] | max d [m] | lost periods | kites ever lost | commands dropped |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['row']} | {r['rms_d']:.4g} | {r['max_d']:.4g} | {r['lost_fraction']:.4g} | "
              f"{int(r['ever_lost'])} of {r['B']} | {r['cmd_dropped']} of {r['cmds']} |")


if __name__ == "__main__":
    a = sys.argv[1:]
    B, episodes, steps = (int(a[0]) if a else 256), (int(a[1]) if len(a) > 1 else 12), (int(a[2]) if len(a) > 2 else 40)
    table([fly(name, B, episodes, steps, mean, dev, comp) for name, mean, dev, comp in ROWS])
