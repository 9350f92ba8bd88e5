"""The 0.1 s question under the transport rule: the closed-loop score of the
kites of tools/delay_study.py (same fleet, seeds, launch states and episodes)
behind a command line that is a pure transport delay.

    python tools/delay_rule_study.py [B] [episodes] [episode_steps]

A row is the plant's actuation delay (fleet.ActuationDelay(rule="transport"):
mean +- deviation, seconds), config.delay, the delay the controller
compensates, and the compensation: "last" predicts the whole delay under the
previous u(t0), "queue" under the commands still in the line
(FleetLoop(delay_comp="queue"), kite_nmpc_set_inflight_device):

  0.1 / 0                 the node's delay, uncompensated
  0.1 / 0.1 last          the node: delay and its compensation
  0.1 / 0.1 queue         the same delay, the queue-aware compensation
  0.1+-0.005 / 0.1 queue  with the injector's jitter
  0.15 / 0.15 last, queue three periods
  0.05 / 0.05 queue       one period: the window holds one command from its
                          start, so this row is delay_study.py's 0.05 / 0.05

One JSON line per row (EpisodeScore.summary plus "cmd_dropped" and "cmds"),
then the table.
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
ROWS = [("0.1 / 0", 0.1, 0.0, 0.0, "last"), ("0.1 / 0.1 last", 0.1, 0.0, 0.1, "last"),
        ("0.1 / 0.1 queue", 0.1, 0.0, 0.1, "queue"), ("0.1+-0.005 / 0.1 queue", 0.1, 0.005, 0.1, "queue"),
        ("0.15 / 0.15 last", 0.15, 0.0, 0.15, "last"), ("0.15 / 0.15 queue", 0.15, 0.0, 0.15, "queue"),
        ("0.05 / 0.05 queue", 0.05, 0.0, 0.05, "queue")]


def fly(name, B, episodes, steps, mean, deviation, comp, how):
    cfg = ok.default_config(N=N, delay=comp, delay_steps=16)
    ctx = ok.BatchNMPC(ok.load_properties(), cfg, B)
    try:
        x0 = synthetic_x0(B, 0, ctx)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        delay = ActuationDelay(B, mean, deviation, seed=81, device="cuda", rule="transport")
        plant = GpuPlant(ctx, cfg.dt / 2, 2, 4, delay=delay)
        score = EpisodeScore(B, device="cuda")
        loop = FleetLoop(GpuStepper(ctx), torch.from_numpy(x0).cuda(), N, cfg.dt, plant=plant, scorer=score,
                         delay_comp=how)
        dropped = torch.zeros((), dtype=torch.int64, device="cuda")
        bad = torch.zeros((), dtype=torch.int64, device="cuda")
        for e in range(episodes):
            if e:
                loop.restart()
            for _ in range(steps):                      # nothing here waits for the device
                loop.step()
                dropped += ((loop.plant_status & ok.PLANT_CMD_DROPPED) != 0).sum()
                bad += ((loop.status & ok.ST_BAD_INFLIGHT) != 0).sum()
        s = score.summary()
        out = dict(row=name, B=B, episodes=episodes, episode_steps=steps, plant_delay=mean, plant_delay_dev=deviation,
                   config_delay=comp, delay_comp=how, rule="transport", cmd_dropped=int(dropped.item()),
                   bad_inflight=int(bad.item()), cmds=B * episodes * steps, **s)
        print(json.dumps(out), flush=True)
        return out
    finally:
        ctx.use_own_stream()
        ctx.close()


def table(rows):
    print("| plant delay / config.delay [s], compensation | rms d [m] | max d [m] | lost periods | kites ever lost | commands dropped |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['row']} | {r['rms_d']:.4g} | {r['max_d']:.4g} | {r['lost_fraction']:.4g} | "
              f"{int(r['ever_lost'])} of {r['B']} | {r['cmd_dropped']} of {r['cmds']} |")


if __name__ == "__main__":
    a = sys.argv[1:]
    B, episodes, steps = (int(a[0]) if a else 256), (int(a[1]) if len(a) > 1 else 12), (int(a[2]) if len(a) > 2 else 40)
    table([fly(name, B, episodes, steps, mean, dev, comp, how) for name, mean, dev, comp, how in ROWS])
