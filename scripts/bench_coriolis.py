#!/usr/bin/env python3
"""Cost of the plant step under the Coriolis stage (brov_coriolis_*).

1. The plant step at B = 16 384 and 262 144 with the stage off, with the rigid-body group and with both groups, taking turns on the same run,
   for three settings of the other stages: none (stage off: plant_kernel), a constant current (stage off: plant_current_kernel<false, false>),
   and thruster stage + periodic wrench + constant current (stage off: plant_current_kernel<true, true>).  `--steps` plant steps enqueued
   back to back between two HIP events, no host wait in between; median of `--repeats` trains after one warm-up round, microseconds per step.
   With the stage off the launches are the parent's, instruction for instruction (profiles/coriolis_isa.txt): the stage-off column of the same
   run is the baseline.  With the stage on, brov_coriolis_last_seconds (two HIP events around ONE launch) is reported beside the train figure,
   and brov_current_last_seconds with the stage off and a current on: plant_current_kernel's single launch on the same run.
   Per instance the stage adds 24 B read (the three added masses, in a row the step reads anyway) and 32 B of "last" written, and about 40 FP64
   operations per RK stage; plant_coriolis_kernel always projects a wrench and a current, zeros where they are off.
2. brov_closed_loop_dob, 64 ticks at B = 4096, N = 20, stage off (the parent's loop) against on (rigid group): ms per tick.

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
        stages = [("plain", False, False, False), ("current", False, False, True), ("thrusters_wrench_current", True, True, True)]
        forms = [(f"{st}/{co}", th, wr, cu, co) for st, th, wr, cu in stages for co in ("off", "rigid", "both")]
        us = {f[0]: [] for f in forms}
        single = {f[0]: [] for f in forms if f[4] != "off" or f[3]}
        for rep in range(a.repeats + 1):
            for name, th, wr, cu, co in forms:
                s.set_plant_wrench(periodic=dict(seed=1)) if wr else s.plant_wrench_off()
                s.set_thrusters(lo=-1540.0, hi=1540.0, gain=gain, onset=onset) if th else s.thrusters_off()
                s.set_current(constant=vc) if cu else s.current_off()
                s.coriolis_off() if co == "off" else s.set_coriolis(rigid=True, added=co == "both")
                s.set_x0(x0); s.plant_wrench_seek(0)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    s.plant_step(0.05 / a.steps, 1)      # (a short step: the state stays where it is over the train)
                e1.record(); torch.cuda.synchronize()
                if rep:                                   # the first round warms up
                    us[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)
                    if co != "off":
                        single[name].append(s.coriolis_last_seconds() * 1e6)
                    elif cu:                              # plant_current_kernel's own two events: the single-launch baseline of the same run
                        single[name].append(s.current_last_seconds() * 1e6)
        row = {"batch": B}
        for name, _, _, _, co in forms:
            row[name] = {"us_per_step_median": float(np.median(us[name])), "us_per_step_min": float(np.min(us[name])),
                         "us_per_step_max": float(np.max(us[name]))}
            if name in single:
                row[name]["us_last_launch_median"] = float(np.median(single[name]))
            if co != "off":
                row[name]["over_off"] = row[name]["us_per_step_median"] / row[name.split("/")[0] + "/off"]["us_per_step_median"]
        kernels.append(row)
        s.close()
    # ---- the DOB loop with the stage off and on -------------------------------------------------------------------------------------
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
            s.set_coriolis(rigid=True)
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
    print(json.dumps({"metric": "plant step under the Coriolis stage, us per step; DOB loop with the stage off and on, ms per tick", "steps": a.steps,
                      "repeats": a.repeats, "plant_kernels": kernels, "dob_loop": {"batch": B, "N": N, "ticks": K, **loops}}))


if __name__ == "__main__":
    main()
