#!/usr/bin/env python3
"""Cost of the plant's delay stage (brov_delay_*).

1. At B = 16 384 and 262 144, on the same run: the plant step with the stage off (plant_kernel: the library's kernel before the stage existed),
   the plant step with the stage on (delay_shift_kernel ahead of the same plant_kernel; delays cycling 0 ... 3, comp = 2), and one launch of
   each of the stage's kernels by the library's own HIP events (brov_delay_last_seconds: the shift of the last plant step, the predictor of
   the last solve).  `--steps` plant steps enqueued back to back between two HIP events, no host wait in between; the forms take turns inside
   every repeat, so that a drift of the machine meets all of them; median of `--repeats` trains after one warm-up round, microseconds per step.
   Per instance the shift reads a 104 B record, 4 B of delay and an 80 B slot and writes an 80 B slot and a 104 B record; the predictor reads
   96 B of state, 128 B of parameters and comp x 32 B of inputs, writes 96 B and does comp x ~600 FP64 operations.
2. brov_closed_loop_dob, 64 ticks at B = 4096, N = 20, with the stage on (delay 2, comp 2) and off, taking turns: ms per tick.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="16384,262144")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--loop-batch", type=int, default=4096)
    ap.add_argument("--loop-ticks", type=int, default=64)
    a = ap.parse_args()
    import torch
    import bluerov2_amd as ba
    from bench import synthetic_inputs
    N, comp = 20, 2
    kernels = []
    for B in [int(b) for b in a.batch.split(",")]:
        x0, circ = synthetic_inputs(B, seed=3, noise=False)
        s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1))); s.set_yref(circ[:N + 1])
        s.solve(sync=True)                      # an input for the plant to hold
        delay = np.arange(B) % 4
        us = {"off": [], "on": []}
        single = {"shift": [], "predict": []}
        for rep in range(a.repeats + 1):
            for name in ("off", "on"):
                s.set_delay(delay, comp=comp) if name == "on" else s.delay_off()
                s.set_x0(x0)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    s.plant_step(0.05 / a.steps, 1)      # (a short step: the state stays where it is over the train)
                e1.record(); torch.cuda.synchronize()
                if name == "on":
                    s.set_x0(x0); s.solve(sync=True)     # one solve behind the predictor
                if rep:                                   # the first round warms up
                    us[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)
                    if name == "on":
                        sh, pr = s.delay_last_seconds()
                        single["shift"].append(sh * 1e6); single["predict"].append(pr * 1e6)
        row = {"batch": B, "comp": comp}
        for name in us:
            row[name] = {"us_per_step_median": float(np.median(us[name])), "us_per_step_min": float(np.min(us[name])),
                         "us_per_step_max": float(np.max(us[name]))}
        row["on_over_off"] = row["on"]["us_per_step_median"] / row["off"]["us_per_step_median"]
        for name in single:
            row[name + "_us_last_launch"] = {"median": float(np.median(single[name])), "min": float(np.min(single[name])),
                                             "max": float(np.max(single[name]))}
        kernels.append(row)
        s.close()
    # ---- the DOB loop with the stage on and off ------------------------------------------------------------------------------
    B, K = a.loop_batch, a.loop_ticks
    x0, circ = synthetic_inputs(B, seed=2, noise=False)
    ep = ba.EkfParams.default(); ep.compensate_coef = 1.0; ep.rotor_constant = 1.0
    for j in range(12, 24):
        ep.K[j] = 0.0
    loops = {}
    solvers = {}
    for name in ("off", "on"):
        s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1))); s.set_trajectory(circ)
        if name == "on":
            s.set_delay(2, comp=comp, observer_applied=True)
        e = ba.BatchEkf(B, ep)
        s.closed_loop_dob(e, ticks=5, line0=0, log=False)
        solvers[name] = (s, e, [])
    for rep in range(3):                                   # the two take turns
        for name, (s, e, dts) in solvers.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            s.closed_loop_dob(e, ticks=K, line0=5 + rep * K, log=False)
            dts.append((time.perf_counter() - t0) / K)
    for name, (s, e, dts) in solvers.items():
        dt = float(np.median(dts))
        loops[name] = {"ticks_per_s": B / dt, "ms_per_tick": dt * 1e3, "ms_per_tick_all": [d * 1e3 for d in dts],
                       "status_nonzero": int((s.results()["status"] != 0).sum())}
        e.close(); s.close()
    loops["on_over_off_ms_per_tick"] = loops["on"]["ms_per_tick"] / loops["off"]["ms_per_tick"]
    print(json.dumps({"metric": "plant step behind the delay stage, us per step; one shift and one predict launch, us; DOB loop with the stage on "
                                "and off, ms per tick", "steps": a.steps, "repeats": a.repeats, "kernels": kernels,
                      "dob_loop": {"batch": B, "N": N, "ticks": K, **loops}}))


if __name__ == "__main__":
    main()
