#!/usr/bin/env python3
"""dev: what the select kernels cost, one JSON line of medians (us) -- for an A/B of two builds of the library, run alternately
(profiles/select_refactor.txt).  Per group shape (ranks x instances per rank on ONE device, copy collective) and gather mode: the select
kernel by its events (SolverGroup.last_seconds()["select"]) and the wall time of gather + select_best; the fleet's select kernel at
V x C = 64 x 64; the wall time of BatchSolver.select_best at B = 4096 and 65536."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bluerov2_amd as ba  # noqa: E402

N, TS, REPS = 20, 0.05, 60


def med_us(v):
    return round(float(np.median(v)) * 1e6, 2)


out = {}
for W, per_rank in ((8, 8192), (1, 4096)):
    total = W * per_rank
    g = ba.SolverGroup([0] * W, total, ba.SolverOptions(N, TS), collective="copy")
    rng = np.random.default_rng(3)
    x0 = np.zeros((total, 12)); x0[:, 0] = 2.0; x0[:, 2] = -20.0
    g.set_x0(x0); g.set_params(ba.P_NOMINAL)
    g.set_candidate_params("lemniscate", rng.uniform(1, 3, total), rng.uniform(0.25, 0.75, total), rng.uniform(0, 2 * np.pi, total))
    g.set_yref_candidates_tick(0.0, TS); g.solve(); g.synchronize()
    for mode, name in ((ba.GATHER_RECORDS, "records"), (ba.GATHER_PACKED, "packed")):
        kern, wall = [], []
        for k in range(REPS + 10):
            g.synchronize()
            t0 = time.perf_counter()
            g.gather(mode); idx, _ = g.select_best()
            t1 = time.perf_counter()
            if k >= 10:
                wall.append(t1 - t0); kern.append(g.last_seconds()["select"])
        out[f"group_{W}x{per_rank}_{name}"] = dict(select_kernel_us=med_us(kern), gather_select_wall_us=med_us(wall), index=idx)
    g.close()

V = C = 64
s = ba.BatchSolver(V * C, ba.SolverOptions(N, TS)); s.set_params(ba.P_NOMINAL); s.solve(sync=True)
f = ba.Fleet(s, C)
t = []
for k in range(REPS + 10):
    f.select(with_records=False)
    if k >= 10:
        t.append(f.last_seconds())
out["fleet_64x64_select_kernel_us"] = med_us(t)
f.close(); s.close()

for B in (4096, 65536):
    s = ba.BatchSolver(B, ba.SolverOptions(N, TS)); s.set_params(ba.P_NOMINAL); s.solve(sync=True)
    t = []
    for k in range(REPS + 10):
        t0 = time.perf_counter(); s.select_best(); t1 = time.perf_counter()
        if k >= 10:
            t.append(t1 - t0)
    out[f"select_best_B{B}_wall_us"] = med_us(t)
    s.close()
print(json.dumps(out))
