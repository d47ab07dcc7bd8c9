#!/usr/bin/env python3
"""Cost of the plant's rotor stage (brov_rotor_*).

1. At B = 16 384 and 262 144, on the same run: the plant step with every stage off (plant_kernel alone), with the rotor stage on
   (rotor_shift_kernel ahead of the same plant_kernel; tau = 0.2 s) and with the delay stage on (delay_shift_kernel ahead of it; delays cycling
   0 ... 3), and one launch of either shift kernel by the library's own HIP events (brov_rotor_last_seconds, brov_delay_last_seconds: the
   shift of the last plant step).  `--steps` plant steps enqueued back to back between two HIP events, no host wait in between; the forms take
   turns inside every repeat, so that a drift of the machine meets all of them; median of `--repeats` trains after one warm-up round,
   microseconds per step.  Per instance the rotor shift reads a 104 B record, 48 B of state and two 48 B coefficient rows and 8 B of lag_sq and
   writes a 104 B record, 48 B of state, 48 B of `last` and 8 B of lag_sq: about 460 B; the delay shift reads a 104 B record, 4 B of delay and
   an 80 B slot and writes an 80 B slot and a 104 B record: about 370 B.
2. brov_closed_loop_dob, 64 ticks at B = 4096, N = 20, with the rotor stage on (tau = 0.2 s, the observer fed the applied thrusts) and off,
   taking turns: ms per tick.

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
    N = 20
    h = 0.05 / a.steps                          # a short step: the state stays where it is over the train
    kernels = []
    for B in [int(b) for b in a.batch.split(",")]:
        x0, circ = synthetic_inputs(B, seed=3, noise=False)
        s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1))); s.set_yref(circ[:N + 1])
        s.solve(sync=True)                      # an input for the plant to hold
        delay = np.arange(B) % 4
        us = {"off": [], "rotor": [], "delay": []}
        single = {"rotor": [], "delay": []}
        for rep in range(a.repeats + 1):
            for name in us:
                s.rotor_off(); s.delay_off()
                if name == "rotor":
                    s.set_rotors(0.2, h=h)
                elif name == "delay":
                    s.set_delay(delay)
                s.set_x0(x0)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    s.plant_step(h, 1)
                e1.record(); torch.cuda.synchronize()
                if rep:                                   # the first round warms up
                    us[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)
                    if name == "rotor":
                        single[name].append(s.rotor_last_seconds() * 1e6)
                    elif name == "delay":
                        single[name].append(s.delay_last_seconds()[0] * 1e6)
        row = {"batch": B}
        for name in us:
            row[name] = {"us_per_step_median": float(np.median(us[name])), "us_per_step_min": float(np.min(us[name])),
                         "us_per_step_max": float(np.max(us[name]))}
        row["rotor_over_off"] = row["rotor"]["us_per_step_median"] / row["off"]["us_per_step_median"]
        for name in single:
            row[name + "_shift_us_last_launch"] = {"median": float(np.median(single[name])), "min": float(np.min(single[name])),
                                                   "max": float(np.max(single[name]))}
        row["rotor_shift_over_delay_shift"] = row["rotor_shift_us_last_launch"]["median"] / row["delay_shift_us_last_launch"]["median"]
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
            s.set_rotors(0.2, observer_applied=True)
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
    print(json.dumps({"metric": "plant step behind the rotor stage, behind the delay stage and with neither, us per step; one rotor shift and one "
                                "delay shift launch, us; DOB loop with the rotor stage on and off, ms per tick", "steps": a.steps,
                      "repeats": a.repeats, "kernels": kernels, "dob_loop": {"batch": B, "N": N, "ticks": K, **loops}}))


if __name__ == "__main__":
    main()
