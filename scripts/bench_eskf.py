#!/usr/bin/env python3
"""Throughput of the batched error-state filter (brov_eskf_*): B filters, ticks on resident inputs, at several batch sizes, for the predict-only
and the update tick -- and ekf_update_kernel_sp (the 18-state observer, brov_ekf_update_device) timed at the same sizes in the same run, as the
yardstick: the tick evaluates no RK4 map and should not be slower per filter.

Prints one JSON line: per batch, updates/s (filters per second, HIP events around the kernel, median of 10), microseconds per launch and the
algorithmic HBM bytes per update against the 6.0-6.3 TB/s a streaming kernel reaches on this part (6.15 TB/s is taken as the reference).  The
covariance is 3.5 KB per filter: only batches beyond the 256 MB Infinity Cache (B = 262 144: 0.9 GB) measure HBM rather than the cache.
--out FILE also writes the line there (profiles/eskf_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_STREAM = 6.15e12
BYTES_UPDATE = 2 * 441 * 8 + 2 * 22 * 8 + (6 + 3 + 3 + 4 + 6) * 8 + (3 + 3 + 4) * 8 + 4      # P and x in and out, the inputs, the outputs
BYTES_PREDICT = 2 * 441 * 8 + 2 * 22 * 8 + 6 * 8 + (3 + 3 + 4) * 8 + 4
BYTES_EKF = 2 * 324 * 8 + 2 * 18 * 8 + (6 + 12 + 6) * 8 + (6 + 4) * 8 + 4


def median_seconds(tick, seconds, n=10):
    t = []
    for _ in range(n):
        tick()
        t.append(seconds())
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="4096,16384,262144", help="comma-separated batch sizes")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bluerov2_amd as ba
    runs = []
    for B in [int(b) for b in a.batch.split(",")]:
        rng = np.random.default_rng(0)
        e = ba.BatchEskf(B)
        x0 = np.zeros(22); x0[6] = 1.0; x0[18] = -9.81
        A = rng.normal(size=(21, 21)) * 0.1
        e.reset(x0, A @ A.T + np.eye(21) * 0.05)
        dev = lambda v: torch.tensor(v, device="cuda")      # noqa: E731
        imu = dev(np.tile([0.0, 0.0, 9.81, 0.0, 0.0, 0.0], (B, 1)) + rng.normal(size=(B, 6)) * 0.01)
        gps_p, gps_v = dev(rng.normal(size=(B, 3)) * 0.05), dev(rng.normal(size=(B, 3)) * 0.05)
        qm = dev(np.tile([1.0, 0.0, 0.0, 0.0], (B, 1)) + rng.normal(size=(B, 4)) * 0.01)
        thrust = dev(rng.uniform(-1, 1, (B, 6)))
        upd = lambda: e.update_device(imu.data_ptr(), gps_p.data_ptr(), gps_v.data_ptr(), qm.data_ptr(), thrust.data_ptr())      # noqa: E731
        pre = lambda: e.predict_device(imu.data_ptr())      # noqa: E731
        for _ in range(a.warmup):
            upd(); pre()
        t_upd = median_seconds(upd, e.last_update_seconds)
        t_pre = median_seconds(pre, e.last_update_seconds)
        st = e.outputs()[3]
        e.close()
        k = ba.BatchEkf(B)
        th, y12, acc = dev(rng.uniform(-1, 1, (B, 6))), dev(rng.normal(size=(B, 12)) * 0.01 + np.array([0, 0, -20.0] + [0.0] * 9)), dev(rng.normal(size=(B, 6)) * 0.01)
        ekf = lambda: k.update_device(th.data_ptr(), y12.data_ptr(), acc.data_ptr())      # noqa: E731
        for _ in range(a.warmup):
            ekf()
        t_ekf = median_seconds(ekf, k.last_update_seconds)
        k.close()
        runs.append({"batch": B,
                     "update": {"updates_per_s": B / t_upd, "us_per_launch": t_upd * 1e6, "hbm_gbs": BYTES_UPDATE * B / t_upd / 1e9,
                                "hbm_frac": BYTES_UPDATE * B / t_upd / HBM_STREAM},
                     "predict_only": {"updates_per_s": B / t_pre, "us_per_launch": t_pre * 1e6, "hbm_gbs": BYTES_PREDICT * B / t_pre / 1e9,
                                      "hbm_frac": BYTES_PREDICT * B / t_pre / HBM_STREAM},
                     "ekf18_update_kernel_sp": {"updates_per_s": B / t_ekf, "us_per_launch": t_ekf * 1e6, "hbm_gbs": BYTES_EKF * B / t_ekf / 1e9},
                     "eskf_update_over_ekf18_time_per_filter": t_upd / t_ekf, "state_mb": (441 + 22) * 8 * B / 1e6,
                     "status_nonzero": int((st != 0).sum())})
        del imu, gps_p, gps_v, qm, thrust, th, y12, acc
    top = runs[-1]
    out = {"metric": "error-state filter update ticks/s (21 error states, 12 measurements)", "value": top["update"]["updates_per_s"],
           "unit": "updates/s", "batch": top["batch"], "us_per_launch": top["update"]["us_per_launch"],
           "roofline_hbm": {"achieved": top["update"]["hbm_gbs"], "peak": HBM_STREAM / 1e9, "unit": "GB/s", "frac": top["update"]["hbm_frac"],
                            "bytes_per_update": BYTES_UPDATE, "bytes_per_predict": BYTES_PREDICT},
           "batches": runs}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
