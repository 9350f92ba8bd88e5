"""Tables for tests/cpp/delay_line_check.cpp, written by the Python models of
tests/delay_rule_ref.py: sends under both arrival rules (drops, bad tau,
coasting periods, falling latencies), schedule rows of lines in every state
(NaN counts, non-finite entries, arrivals before, inside, at and beyond the
window) and substep counts.  Doubles are written as C99 hex floats.

  python tools/delay_line_tables.py tables.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import delay_ref as dr            # noqa: E402
import delay_rule_ref as rr       # noqa: E402

H, STEPS, SUB = 0.02, 3, 2
DT = STEPS * H


def hx(v):
    v = float(v)
    if v != v:
        return "nan"
    if v in (float("inf"), float("-inf")):
        return "inf" if v > 0 else "-inf"
    return v.hex()


def main(path):
    rng = np.random.default_rng(20261021)
    out = ["# written by tools/delay_line_tables.py"]
    nrows = 0
    for rule in (0.0, 1.0, float("nan"), 2.0):
        for regime in range(6):
            ln, t = rr.Line(rule), float(rng.uniform(0.0, 3.0))
            for p in range(40):
                if regime == 0:
                    tau = 2 * DT                                    # the node's two periods
                elif regime == 1:
                    tau = 2 * DT * (1 + 0.1 * rng.uniform(-1, 1))
                elif regime == 2:
                    tau = 4.7 * DT                                  # the depth overflows
                elif regime == 3:
                    tau = [3.2, 2.1, 1.0, 0.3, 0.0][p % 5] * DT     # falling
                elif regime == 4:
                    tau = rng.choice([0.0, 0.5 * H, DT, -0.01, np.nan, np.inf])
                else:
                    tau = rng.uniform(0.0, 6 * DT)
                has = not (regime >= 3 and rng.uniform() < 0.25)
                u = rng.uniform(-0.2, 0.2, 4)
                before = ln.as_row()
                bits = ln.send(u, tau, t) if has else 0
                after = ln.as_row()
                out.append(" ".join(["send"] + [hx(v) for v in before] + [hx(v) for v in u] +
                                    [hx(tau), hx(t), hx(1.0 if has else 0.0)] + [hx(v) for v in after] +
                                    [hx(len(ln.fifo)), hx(bits)]))
                # the schedule of the line as it stands, seen now and a little later
                for t_seen in (t, t + 0.3 * DT):
                    row = ln.as_row()
                    out.append(" ".join(["row"] + [hx(v) for v in row] + [hx(t_seen)] +
                                        [hx(v) for v in rr.inflight_row(row, t_seen)]))
                    nrows += 1
                for tk in dr.tick_times(t, H, STEPS, SUB):
                    ln.tick(tk)
                t += DT
    # rows the flight never produces
    for _ in range(400):
        row = rng.uniform(-1.0, 1.0, dr.NLINE)
        row[dr.COUNT] = rng.choice([0.0, 1.0, 2.0, 3.0, 4.0, 7.0, 0.5, -3.0, np.nan, np.inf, 1e300])
        row[dr.T_ARR:dr.T_ARR + 4] = rng.uniform(0.0, 0.4, 4)
        for _ in range(int(rng.integers(0, 3))):
            row[int(rng.integers(0, dr.NLINE))] = rng.choice([np.nan, np.inf, -np.inf])
        t_seen = float(rng.uniform(0.0, 0.3))
        out.append(" ".join(["row"] + [hx(v) for v in row] + [hx(t_seen)] + [hx(v) for v in rr.inflight_row(row, t_seen)]))
    for D, steps in ((0.1, 16), (0.15, 16), (0.05, 16), (0.1, 1), (0.1, 64), (0.07, 5)):
        h_max = D / steps
        lens = [D, 0.0, h_max, np.nextafter(h_max, 0.0), np.nextafter(h_max, 1.0), 2 ** -56, 3 * D]
        lens += [k * h_max for k in range(steps + 2)] + list(rng.uniform(0.0, D, 40))
        for L in lens:
            out.append(" ".join(["sub", hx(L), hx(h_max), hx(steps), hx(rr.substeps(L, h_max, steps))]))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print(f"{path}: {len(out) - 1} records")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "delay_line_tables.txt")
