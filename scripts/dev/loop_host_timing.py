#!/usr/bin/env python3
"""dev: the host cost of the closed loops, one JSON line of medians (us per call) -- for an A/B of two builds of the library, run
alternately in fresh processes (profiles/wrench_logs_refactor.txt).  Wall clock around the call, with logs, after a warm-up, from the same
start every time: closed_loop at B = 64, N = 20, 50 ticks under the periodic wrench (a launch per step) and under mode OFF (one launch),
closed_loop_dob at the same shape, Fleet.closed_loop_dob at V = 16, C = 4 with an observer."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bluerov2_amd as ba  # noqa: E402
from oracle import trajectory_oracle as T  # noqa: E402

N, B, V, C, TICKS, REPS, WARM = 20, 64, 16, 4, 50, 50, 5
PERIODIC = dict(seed=0xC0FFEE123456789, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)


def ekf(batch):
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
    return ba.BatchEkf(batch, par)


def median_us(prepare, call):
    t = []
    for k in range(REPS + WARM):
        prepare()
        t0 = time.perf_counter(); call(); t1 = time.perf_counter()
        if k >= WARM:
            t.append(t1 - t0)
    return round(float(np.median(t)) * 1e6, 1)


out = {}
traj = T.circle()
rng = np.random.default_rng(2)
x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
s = ba.BatchSolver(B, ba.SolverOptions(N))
s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1))); s.set_trajectory(traj)
e = ekf(B)


def restart():
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.init_iterate_default(); s.plant_wrench_seek(0)


s.set_plant_wrench(periodic=PERIODIC)
out["closed_loop_per_step_us"] = median_us(restart, lambda: s.closed_loop(TICKS, log_wrench=True))
out["closed_loop_dob_us"] = median_us(restart, lambda: s.closed_loop_dob(e, ticks=TICKS))
s.plant_wrench_off()
out["closed_loop_one_launch_us"] = median_us(restart, lambda: s.closed_loop(TICKS, log_wrench=True))
s.close(); e.close()

s = ba.BatchSolver(V * C, ba.SolverOptions(N, 0.05))
s.set_candidate_params("circle", np.tile(2.0 + 0.5 * np.arange(C) / C, V), np.full(V * C, 0.5), np.zeros(V * C))
xv = np.zeros((V, 12)); xv[:, 0] = -2.2; xv[:, 2] = -20.0; xv[:, 5] = -0.5 * np.pi; xv[:, :3] += rng.normal(size=(V, 3)) * 0.1
f = ba.Fleet(s, C)
f.set_plant_params(np.tile(ba.P_NOMINAL, (V, 1))); f.set_wrench(periodic=PERIODIC)
e = ekf(V)


def restart_fleet():
    s.set_params(ba.P_NOMINAL); s.init_iterate_default(); f.set_state(xv); f.wrench_seek(0)


out["fleet_closed_loop_dob_us"] = median_us(restart_fleet, lambda: f.closed_loop_dob(e, TICKS))
f.close(); s.close(); e.close()
print(json.dumps(out))
