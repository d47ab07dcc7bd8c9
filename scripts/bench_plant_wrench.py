#!/usr/bin/env python3
"""Cost of the plant under a world-frame wrench and of the DOB loop as one call.

1. plant_wrench_kernel in its three modes beside plant_kernel (mode OFF) on the same run, at B = 4096 and 16 384: `--steps` plant steps
   enqueued back to back between two HIP events, no host wait in between; median of `--repeats` such trains, microseconds per step.
   One step reads 240 B (+ 48 B of wrench in constant mode, 8 B of gain in table mode) and writes 96 B per instance: at these batches a
   few microseconds of HBM time, about what a launch costs -- a wrench kernel that takes as long as plant_kernel hides its per-stage
   projection (and the periodic mode its sin and three hashes) behind that.
2. brov_closed_loop_dob beside the loop it replaces, five calls per tick from Python (bench.py, config 3: window, RTI step, plant step,
   EKF update, hand-off), B = 16 384, N = 20, under the periodic wrench: ticks per second (instances x ticks / s) and ms per tick.

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
    ap.add_argument("--batch", default="4096,16384")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--loop-batch", type=int, default=16384)
    ap.add_argument("--loop-ticks", type=int, default=40)
    a = ap.parse_args()
    import torch
    import bluerov2_amd as ba
    from bench import synthetic_inputs
    tab = np.load(os.path.join(ROOT, "tests", "golden", "wrench_tables.npz"))["table"]
    N = 20
    kernels = []
    for B in [int(b) for b in a.batch.split(",")]:
        rng = np.random.default_rng(B)
        x0, circ = synthetic_inputs(B, seed=3, noise=False)
        s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1))); s.set_yref(circ[:N + 1])
        s.solve(sync=True)                      # an input for the plant to hold
        row = {"batch": B}
        modes = [("off_plant_kernel", None), ("constant", dict(constant=rng.uniform(-10, 10, (B, 6)))),
                 ("periodic", dict(periodic=dict(seed=1))), ("table", dict(table=tab, gain=rng.uniform(0.5, 1.5, B)))]
        for name, kw in modes:
            s.plant_wrench_off() if kw is None else s.set_plant_wrench(**kw)
            us = []
            for rep in range(a.repeats + 1):
                s.set_x0(x0); s.plant_wrench_seek(0)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    s.plant_step(0.05 / a.steps, 1)      # (a short step: the state stays where it is over the train)
                e1.record(); torch.cuda.synchronize()
                if rep:                                   # the first train warms up
                    us.append(e0.elapsed_time(e1) * 1e3 / a.steps)
            row[name] = {"us_per_step_median": float(np.median(us)), "us_per_step_min": float(np.min(us)), "us_per_step_max": float(np.max(us))}
        kernels.append(row)
        s.close()
    # ---- the DOB loop: one call against five calls per tick ------------------------------------------------------------------
    B, K = a.loop_batch, a.loop_ticks
    x0, circ = synthetic_inputs(B, seed=2, noise=False)
    ep = ba.EkfParams.default(); ep.compensate_coef = 1.0; ep.rotor_constant = 1.0
    for j in range(12, 24):
        ep.K[j] = 0.0
    loops = {}
    for name in ("five_calls_per_tick", "closed_loop_dob"):
        s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1))); s.set_trajectory(circ)
        s.set_plant_wrench(periodic=dict(seed=2))
        e = ba.BatchEkf(B, ep)

        def run(line0, ticks):
            if name == "closed_loop_dob":
                s.closed_loop_dob(e, ticks=ticks, line0=line0, log=False)
            else:
                for k in range(ticks):
                    s.set_yref_from_trajectory(line0 + k, 16); s.solve(); s.plant_step(0.05, 1); e.update_from_solver(s); e.apply_to_solver(s)
                torch.cuda.synchronize()
        run(0, 5)
        dts = []
        for rep in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            run(5 + rep * K, K)
            dts.append((time.perf_counter() - t0) / K)
        dt = float(np.median(dts))
        loops[name] = {"ticks_per_s": B / dt, "ms_per_tick": dt * 1e3, "ms_per_tick_all": [d * 1e3 for d in dts],
                       "status_nonzero": int((s.results()["status"] != 0).sum())}
        e.close(); s.close()
    print(json.dumps({"metric": "plant step under a world-frame wrench, us per step; DOB loop, instance-ticks per second", "steps": a.steps,
                      "repeats": a.repeats, "plant_kernels": kernels, "dob_loop": {"batch": B, "N": N, "ticks": K, **loops}}))


if __name__ == "__main__":
    main()
