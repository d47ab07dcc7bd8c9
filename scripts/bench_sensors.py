#!/usr/bin/env python3
"""Cost of the sensor stage (brov_sensor_*).

1. The measure kernel at B = 16 384 and 262 144: `--steps` forced refreshes (brov_sensor_measure) enqueued back to back between two HIP events,
   no host wait in between; median of `--repeats` trains after one warm-up round, microseconds per launch.  brov_sensor_last_seconds (two HIP
   events around ONE launch, recorded by the library on every refresh) is reported beside the train figure.  Then the plant step with the
   stage off and on (plant kernel + regular refresh), the two taking turns inside every repeat, microseconds per step.  With the stage off
   the step launches what the library launched before the stage existed: the same run gives the baseline.
   Per instance a refresh reads 96 B of state, 96 B of held measurement, 2 x 96 B of sigma and bias and 8 B of dropout, writes 96 B, reads and
   writes 4 + 96 B of statistics (regular refreshes only), and computes up to 37 counter hashes.
2. brov_closed_loop_dob, 64 ticks at B = 4096, N = 20, with the stage on (noise, bias, quantised position, slow attitude, 5 % dropout) and
   off: ms per tick.  The stage-off loop is the loop of the commit before the stage, launch for launch.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def config(B, rng):
    quant = np.zeros(12); quant[:3] = 0.01
    period = np.ones(12, dtype=np.int32); period[3:6] = 2
    return dict(seed=11, sigma=rng.uniform(0.0, 0.01, (B, 12)), bias=rng.uniform(-0.01, 0.01, (B, 12)), quant=quant, period=period, dropout=0.05)


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
        cfg = config(B, rng)
        us = {"measure": [], "step_off": [], "step_on": []}
        single = []

        def train(call):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                call()
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.steps

        for rep in range(a.repeats + 1):
            s.set_sensors(**cfg); s.set_x0(x0); s.plant_wrench_seek(0)
            t_meas = train(s.sensor_measure)
            one = s.sensor_last_seconds() * 1e6
            t_on = train(lambda: s.plant_step(0.05 / a.steps, 1))      # (a short step: the state stays where it is over the train)
            s.sensors_off(); s.set_x0(x0); s.plant_wrench_seek(0)
            t_off = train(lambda: s.plant_step(0.05 / a.steps, 1))
            if rep:                                   # the first round warms up
                us["measure"].append(t_meas); us["step_on"].append(t_on); us["step_off"].append(t_off); single.append(one)
        row = {"batch": B}
        for name, v in us.items():
            row[name] = {"us_median": float(np.median(v)), "us_min": float(np.min(v)), "us_max": float(np.max(v))}
        row["measure"]["us_last_launch_median"] = float(np.median(single))
        row["step_on_minus_off_us"] = row["step_on"]["us_median"] - row["step_off"]["us_median"]
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
            s.set_sensors(**config(B, np.random.default_rng(1)))
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
    loops["on_minus_off_us_per_tick"] = (loops["on"]["ms_per_tick"] - loops["off"]["ms_per_tick"]) * 1e3
    loops["on_over_off_ms_per_tick"] = loops["on"]["ms_per_tick"] / loops["off"]["ms_per_tick"]
    print(json.dumps({"metric": "sensor stage: measure kernel and plant step, us per launch; DOB loop with the stage on and off, ms per tick",
                      "steps": a.steps, "repeats": a.repeats, "kernels": kernels, "dob_loop": {"batch": B, "N": N, "ticks": K, **loops}}))


if __name__ == "__main__":
    main()
