#!/usr/bin/env python3
"""The fleet planning loop in moving water (brov_vehicle_current_*, brov_vehicle_coriolis_*; fleet_plant_water_kernel; DESIGN.md section
4.12c) beside the same loop with both stages off.

At V x C = 64 x 64 and 256 x 64, N = 20, circle candidates with distinct radii per candidate, planning ticks per second of
brov_closed_loop_fleet (no logs: one host wait per run), all in the same run:
  off               both stages off: the still-water plant kernel, the yardstick of this run
  constant          a constant current per vehicle
  gauss_markov      a Gauss-Markov current per vehicle (the state advances behind every step)
  current_coriolis  a constant current and both groups of the Coriolis stage
  wrench            for comparison only: the periodic world-frame wrench and no water (one more launch per tick, the wrench's evaluation)
The legs are interleaved: every repeat runs each leg once, so a drift of the machine falls on all of them.  Every run starts from the same
states and the same iterate.  Median of `--repeats` runs after one warm-up run each.  Prints one JSON line and writes it to `--out`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("off", "constant", "gauss_markov", "current_coriolis", "wrench")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x64,256x64")
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_water_bench.json"))
    a = ap.parse_args()
    import torch
    import bluerov2_amd as ba
    N, TS, rows = 20, 0.05, []
    for V, C in [tuple(int(t) for t in sh.split("x")) for sh in a.shapes.split(",")]:
        B = V * C
        rng = np.random.default_rng(V)
        radius = np.tile(2.0 + 0.5 * np.arange(C) / C, V)
        xv = np.zeros((V, 12)); xv[:, 0] = -2.2; xv[:, 2] = -20.0; xv[:, 5] = -0.5 * np.pi
        xv[:, :3] += rng.normal(size=(V, 3)) * 0.1
        vc = rng.uniform(-0.4, 0.4, (V, 3)) * np.array([1.0, 1.0, 0.2])
        s = ba.BatchSolver(B, ba.SolverOptions(N, TS))
        s.set_params(ba.P_NOMINAL)
        s.set_candidate_params("circle", radius, np.full(B, 0.5), np.zeros(B))
        f = ba.Fleet(s, C)

        def run(which):
            s.init_iterate_default(); s.set_params(ba.P_NOMINAL); f.reset(); f.set_state(xv)
            f.current_off(); f.coriolis_off(); f.wrench_off()
            if which in ("constant", "current_coriolis"):
                f.set_current(constant=vc)
            if which == "gauss_markov":
                f.set_current(gauss_markov=dict(seed=V, mean=vc, mu=0.5, amp=0.02, lo=-0.6, hi=0.6, step=TS))
            if which == "current_coriolis":
                f.set_coriolis(ba.CORIOLIS_RIGID | ba.CORIOLIS_ADDED)
            if which == "wrench":
                f.set_wrench(periodic=dict(seed=V))
            torch.cuda.synchronize(); t0 = time.perf_counter()
            f.closed_loop(a.ticks, 0.0, TS, TS, 0.05, 1, log=False)
            return time.perf_counter() - t0
        for which in LEGS:
            run(which)
        dts = {which: [] for which in LEGS}
        for _ in range(a.repeats):
            for which in LEGS:
                dts[which].append(run(which))
        row = {"vehicles": V, "candidates": C, "batch": B}
        for which in LEGS:
            med = float(np.median(dts[which]))
            row[which] = {"seconds_median": med, "seconds_min": float(np.min(dts[which])), "seconds_max": float(np.max(dts[which])),
                          "ticks_per_s": a.ticks / med, "us_per_tick": 1e6 * med / a.ticks}
        for which in LEGS[1:]:
            row[which]["us_per_tick_over_off"] = row[which]["us_per_tick"] - row["off"]["us_per_tick"]
        rows.append(row)
        f.close(); s.close()
    out = {"metric": "fleet planning loop in moving water against the same loop with both stages off, planning ticks per second", "N": N,
           "ticks": a.ticks, "repeats": a.repeats, "legs": list(LEGS), "rows": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
