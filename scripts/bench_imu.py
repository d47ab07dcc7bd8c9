#!/usr/bin/env python3
"""The filter at its sensors' rates, timed on one GPU (HIP events around the kernels, median of 10, as scripts/bench_eskf.py):
  * the IMU/GPS stage's refresh (imu_measure_kernel) beside the sensor stage's (sensor_measure_kernel) behind the same plant steps;
  * the masked tick with every filter holding a fix beside the update kernel, and with none beside the predict-only kernel; the margin for
    "equal" is the spread between repeated medians of the update kernel in the same run, which is reported;
  * brov_closed_loop_eskf per control tick (wall clock around the call) beside the same sequence composed from Python and brov_closed_loop_dob.
Prints one JSON line; --out FILE also writes it there (profiles/imu_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_IMU = (12 + 3 + 3 + 12 + 6 + 1) * 8 + 4 + 3 * 4 + (6 + 3 + 3 + 4 + 3 + 3) * 8 + 4 + 4 + 3 * 4      # read; written with a fix and the statistics
BYTES_SENSOR = 688


def median_seconds(tick, seconds, n=10):
    t = []
    for _ in range(n):
        tick()
        t.append(seconds())
    return float(np.median(t))


def stage(ba, B, N=20, h=0.01):
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05), device=0)
    rng = np.random.default_rng(0)
    x0 = np.zeros((B, 12)); x0[:, 2] = -20.0; x0[:, 6:12] = rng.normal(size=(B, 6)) * 0.1
    s.set_x0(x0); s.set_params(ba.P_NOMINAL)
    yref = np.zeros((N + 1, 16)); yref[:, 2] = -20.0
    s.set_yref(yref); s.solve(sync=True)
    s.set_sensors(seed=1, sigma=0.01, dropout=0.1)
    s.set_imu(h, gps_every=1, seed=1, sigma=0.01, bias=0.001, dropout=0.1)
    for _ in range(3):
        s.plant_step(h)
    t_imu = median_seconds(lambda: s.plant_step(h), s.imu_last_seconds)
    t_sen = median_seconds(lambda: s.plant_step(h), s.sensor_last_seconds)
    s.close()
    return {"batch": B, "imu_refresh_us": t_imu * 1e6, "sensor_refresh_us": t_sen * 1e6, "imu_bytes_per_instance": BYTES_IMU,
            "sensor_bytes_per_instance": BYTES_SENSOR, "imu_gbs": BYTES_IMU * B / t_imu / 1e9, "sensor_gbs": BYTES_SENSOR * B / t_sen / 1e9}


def masked(ba, torch, B, warmup=3):
    rng = np.random.default_rng(0)
    e = ba.BatchEskf(B)
    x0 = np.zeros(22); x0[6] = 1.0; x0[18] = -9.81
    A = rng.normal(size=(21, 21)) * 0.1
    e.reset(x0, A @ A.T + np.eye(21) * 0.05)
    dev = lambda v: torch.tensor(v, device="cuda")      # noqa: E731
    imu = dev(np.tile([0.0, 0.0, 9.81, 0.0, 0.0, 0.0], (B, 1)) + rng.normal(size=(B, 6)) * 0.01)
    gp, gv = dev(rng.normal(size=(B, 3)) * 0.05), dev(rng.normal(size=(B, 3)) * 0.05)
    qm = dev(np.tile([1.0, 0.0, 0.0, 0.0], (B, 1)) + rng.normal(size=(B, 4)) * 0.01)
    th = dev(rng.uniform(-1, 1, (B, 6)))
    ones, zeros = torch.ones(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    ptrs = [t.data_ptr() for t in (imu, gp, gv, qm, th)]
    calls = {"update": lambda: e.update_device(*ptrs), "masked_all_fix": lambda: e.tick_device(*ptrs, ones.data_ptr()),
             "predict_only": lambda: e.predict_device(ptrs[0]), "masked_no_fix": lambda: e.tick_device(*ptrs, zeros.data_ptr())}
    for c in calls.values():
        for _ in range(warmup):
            c()
    out = {"batch": B}
    rep = {k: [] for k in calls}
    for _ in range(3):                                   # repeated medians, interleaved
        for k, c in calls.items():
            rep[k].append(median_seconds(c, e.last_update_seconds) * 1e6)
    for k, v in rep.items():
        out[k + "_us"] = float(np.median(v))
        out[k + "_us_medians"] = v
    out["update_spread_us"] = max(rep["update"]) - min(rep["update"])
    out["masked_all_fix_over_update"] = out["masked_all_fix_us"] / out["update_us"]
    out["masked_no_fix_over_predict_only"] = out["masked_no_fix_us"] / out["predict_only_us"]
    e.close()
    return out


def loop(ba, B=4096, N=20, dt=0.05, per_tick=5, ticks=20):
    def pair():
        t = np.arange(N + ticks + 2) * dt
        traj = np.zeros((len(t), 16)); traj[:, 0], traj[:, 1], traj[:, 2] = 2 * np.cos(0.5 * t), 2 * np.sin(0.5 * t), -20.0
        s = ba.BatchSolver(B, ba.SolverOptions(N, dt), device=0)
        x0 = np.zeros((B, 12)); x0[:, 0], x0[:, 2] = 2.0, -20.0
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_trajectory(traj)
        return s
    h = dt / per_tick
    par = ba.EskfParams.default(); par.dt = h; par.compensate_coef = par.rotor_constant = 1.0
    out = {"batch": B, "N": N, "imu_per_tick": per_tick, "ticks": ticks}
    s = pair(); s.set_imu(h, gps_every=3, seed=1, sigma=0.01, dropout=0.1); e = ba.BatchEskf(B, par)
    ba.closed_loop_eskf(s, e, 2, dt=dt, imu_per_tick=per_tick, log=False)
    t0 = time.perf_counter(); ba.closed_loop_eskf(s, e, ticks, line0=2, dt=dt, imu_per_tick=per_tick, log=False)
    out["closed_loop_eskf_us_per_tick"] = (time.perf_counter() - t0) / ticks * 1e6
    t0 = time.perf_counter()
    for k in range(ticks):
        s.set_yref_from_trajectory(k, 16); s.solve()
        for _ in range(per_tick):
            s.plant_step(h); e.tick_from_solver(s)
        e.apply_to_solver(s)
    s.get_x0()
    out["composed_us_per_tick"] = (time.perf_counter() - t0) / ticks * 1e6
    e.close(); s.close()
    s = pair(); k = ba.BatchEkf(B)
    s.closed_loop_dob(k, ticks=2, dt=dt, log=False)
    t0 = time.perf_counter(); s.closed_loop_dob(k, ticks=ticks, line0=2, dt=dt, log=False)
    out["closed_loop_dob_us_per_tick"] = (time.perf_counter() - t0) / ticks * 1e6
    k.close(); s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage-batch", default="16384,262144")
    ap.add_argument("--tick-batch", default="4096,262144")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bluerov2_amd as ba
    out = {"metric": "masked error-state filter tick, every filter holding a fix, over the update kernel (time per launch)",
           "masked_tick": [masked(ba, torch, int(b)) for b in a.tick_batch.split(",")],
           "stage_refresh": [stage(ba, int(b)) for b in a.stage_batch.split(",")], "loop": loop(ba)}
    out["value"], out["unit"] = out["masked_tick"][-1]["masked_all_fix_over_update"], "ratio"
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
