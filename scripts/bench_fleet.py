#!/usr/bin/env python3
"""The fleet planning loop on the device beside the same loop composed on the host (brov_fleet_*, brov_closed_loop_fleet; DESIGN.md
section 4.12).

At V x C = 64 x 64 and 256 x 64, N = 20, circle candidates with distinct radii per candidate:
1. seconds of fleet_select_kernel (brov_fleet_last_seconds: HIP events around the kernel);
2. planning ticks per second of brov_closed_loop_fleet (no logs: one host wait per run);
3. planning ticks per second of the loop composed from Python the way it had to be before: solve -> get_results -> numpy arg-min ->
   plant_step -> set_x0 with the winner's state (104 B x B down, 96 B x B up and two synchronisations per tick);
4. planning ticks per second of brov_closed_loop_fleet_dob under the periodic world-frame wrench per vehicle (brov_vehicle_wrench_periodic),
   without an observer ("wrench") and with an EKF of batch V closing the loop ("wrench_observer"); no logs.
All loops start from the same states and the same iterate.  Median of `--repeats` runs after one warm-up run each.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_argmin(res, V, C):
    """per group the index of the lowest cost among the successful, finite candidates (-1: none); vectorised"""
    cost = np.where((res["status"] == 0) & np.isfinite(res["cost"]), res["cost"], np.inf).reshape(V, C)
    w = np.argmin(cost, axis=1)
    return np.where(np.isfinite(cost[np.arange(V), w]), w, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x64,256x64")
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
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
        s = ba.BatchSolver(B, ba.SolverOptions(N, TS))
        s.set_params(ba.P_NOMINAL)
        s.set_candidate_params("circle", radius, np.full(B, 0.5), np.zeros(B))
        f = ba.Fleet(s, C)
        idx0 = np.arange(V) * C
        # the observer for the device plant (unit scaling, no roll / pitch thrust), as the tests configure it
        par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
        for j in range(12, 24):
            par.K[j] = 0.0
        e = ba.BatchEkf(V, par)

        def run(which):
            s.init_iterate_default(); s.set_params(ba.P_NOMINAL); f.reset(); f.set_state(xv); e.reset()
            if which in ("wrench", "wrench_observer"):
                f.set_wrench(periodic=dict(seed=V)); f.set_plant_params(np.tile(ba.P_NOMINAL, (V, 1)))
            else:
                f.wrench_off(); f.set_plant_params(None)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            if which == "fleet":
                f.closed_loop(a.ticks, 0.0, TS, TS, 0.05, 1, log=False)
            elif which in ("wrench", "wrench_observer"):
                f.closed_loop_dob(e if which == "wrench_observer" else None, a.ticks, 0.0, TS, TS, 0.05, 1, log=False)
            else:
                for k in range(a.ticks):
                    s.set_yref_candidates_tick(0.0 + k * TS, TS); s.solve()
                    w = host_argmin(s.results(), V, C)
                    s.plant_step(0.05, 1)
                    x = s.get_x0()
                    s.set_x0(np.repeat(x[idx0 + np.maximum(w, 0)], C, axis=0))
            return time.perf_counter() - t0
        row = {"vehicles": V, "candidates": C, "batch": B}
        for which in ("fleet", "composed", "wrench", "wrench_observer"):
            run(which)
            dts = [run(which) for _ in range(a.repeats)]
            row[which] = {"seconds_median": float(np.median(dts)), "seconds_min": float(np.min(dts)), "seconds_max": float(np.max(dts)),
                          "ticks_per_s": a.ticks / float(np.median(dts))}
        run("fleet")
        sel = []
        for _ in range(a.repeats):
            f.select(with_records=False)
            sel.append(f.last_seconds())
        row["select_kernel_seconds_median"] = float(np.median(sel))
        row["select_kernel_seconds_min"] = float(np.min(sel))
        row["fleet_over_composed_ticks_per_s"] = row["fleet"]["ticks_per_s"] / row["composed"]["ticks_per_s"]
        # select reads cost + status (16 C); plant reads state, u0, parameters (256) and writes state, held input, status, winner (136);
        # the broadcast writes 96 C
        row["device_bytes_per_vehicle_tick"] = 16 * C + 256 + 136 + 96 * C
        row["host_bytes_per_vehicle_tick_composed"] = (104 + 96 + 96) * C
        # under a wrench: 48 written by the generator and read by the plant.  With the observer: its inputs assembled (176 read, 240
        # written) and read (192), its state read and written (18 + 324 doubles each way), 80 of outputs, and the hand-off (32 read,
        # 32 written per candidate and stage)
        row["device_bytes_per_vehicle_tick_wrench"] = row["device_bytes_per_vehicle_tick"] + 96
        row["device_bytes_per_vehicle_tick_wrench_observer"] = (row["device_bytes_per_vehicle_tick_wrench"] + 416 + 192 + 2 * 2736 + 80 + 32
                                                                + 32 * C * (N + 1))
        rows.append(row)
        f.close(); e.close(); s.close()
    print(json.dumps({"metric": "fleet planning loop on the device against the loop composed on the host, planning ticks per second", "N": N,
                      "ticks": a.ticks, "repeats": a.repeats, "rows": rows}))


if __name__ == "__main__":
    main()
