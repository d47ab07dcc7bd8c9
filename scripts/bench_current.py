#!/usr/bin/env python3
"""Cost of the plant step in moving water (brov_current_*).

1. The plant step at B = 16 384 and 262 144 for every combination of thruster stage and periodic world wrench, in three forms on the same
   run: current off, a constant current, the Gauss-Markov current.  `--steps` plant steps enqueued back to back between two HIP events, no
   host wait in between; the forms take turns inside every repeat, so that a drift of the machine meets all of them; median of `--repeats`
   trains after one warm-up round, microseconds per step.  The current-off forms are the four plant kernels of the parent commit,
   instruction for instruction (profiles/current_isa.txt): the same run on the same box gives the parent's baseline.  With a current on,
   brov_current_last_seconds (two HIP events around ONE launch, recorded by the library on every such step) is reported beside the train
   figure.  Per instance the current adds 24 B read and 24 B of "last applied" written, in Gauss-Markov mode 24 B of mean read and 24 B of
   state written as well, to the step's 240 B in / 96 B out, and 15 FP64 operations per RK stage; without a world wrench the kernel still
   projects a zero wrench (36 operations per stage that add zeros).
2. brov_closed_loop_dob, 64 ticks at B = 4096, N = 20, in still water (the parent's loop) and under a constant current: ms per tick.

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
    kernels = []
    for B in [int(b) for b in a.batch.split(",")]:
        rng = np.random.default_rng(B)
        x0, circ = synthetic_inputs(B, seed=3, noise=False)
        s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1))); s.set_yref(circ[:N + 1])
        s.solve(sync=True)                      # an input for the plant to hold
        gain = rng.uniform(0.5, 1.0, (B, 6))
        onset = rng.integers(0, a.steps, B)
        vc = rng.uniform(-0.4, 0.4, (B, 3))
        stages = [("plain", False, False), ("thrusters", True, False), ("wrench", False, True), ("thrusters_wrench", True, True)]
        forms = [(f"{st}/{cur}", th, wr, cur) for st, th, wr in stages for cur in ("off", "constant", "gauss_markov")]
        us = {name: [] for name, _, _, _ in forms}
        single = {name: [] for name, _, _, cur in forms if cur != "off"}
        for rep in range(a.repeats + 1):
            for name, th, wr, cur in forms:
                s.set_plant_wrench(periodic=dict(seed=1)) if wr else s.plant_wrench_off()
                s.set_thrusters(lo=-1540.0, hi=1540.0, gain=gain, onset=onset) if th else s.thrusters_off()
                if cur == "off":
                    s.current_off()
                elif cur == "constant":
                    s.set_current(constant=vc)
                else:
                    s.set_current(gauss_markov=dict(seed=2, mean=vc, mu=0.5, amp=0.05, lo=-0.4, hi=0.4, step=0.05))   # the launch file's bounds
                s.set_x0(x0); s.plant_wrench_seek(0)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    s.plant_step(0.05 / a.steps, 1)      # (a short step: the state stays where it is over the train)
                e1.record(); torch.cuda.synchronize()
                if rep:                                   # the first round warms up
                    us[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)
                    if cur != "off":
                        single[name].append(s.current_last_seconds() * 1e6)
        row = {"batch": B}
        for name, _, _, cur in forms:
            row[name] = {"us_per_step_median": float(np.median(us[name])), "us_per_step_min": float(np.min(us[name])),
                         "us_per_step_max": float(np.max(us[name]))}
            if cur != "off":
                row[name]["us_last_launch_median"] = float(np.median(single[name]))
                row[name]["over_off"] = row[name]["us_per_step_median"] / row[name.split("/")[0] + "/off"]["us_per_step_median"]
        kernels.append(row)
        s.close()
    # ---- the DOB loop in still and in moving water ------------------------------------------------------------------------------
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
            s.set_current(constant=ba.current_from_angles(0.4, 0.7, 0.0))
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
    print(json.dumps({"metric": "plant step under an ocean current, us per step; DOB loop in still and moving water, ms per tick", "steps": a.steps,
                      "repeats": a.repeats, "plant_kernels": kernels, "dob_loop": {"batch": B, "N": N, "ticks": K, **loops}}))


if __name__ == "__main__":
    main()
