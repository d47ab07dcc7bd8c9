#!/usr/bin/env python3
"""Throughput of the batched RLS-FF parameter estimator of the adaptive MPC loop (brov_rls_*): B estimators (four axes each), K ticks
on resident inputs, at several batch sizes.

Prints one JSON line: per batch, updates/s (instances per second, HIP events around the update kernel), microseconds per launch and
the algorithmic HBM bytes per update against 8 TB/s.  The headline is the largest batch: the state is ~2.4 KB per instance (default
windows), so only batches beyond the 256 MB Infinity Cache (B = 262 144: 0.6 GB) measure HBM rather than the cache."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bytes_per_update(ns, nl):
    """algorithmic HBM traffic of one instance-tick (four axes): theta / P / lambda read and written, F / e / p[0..3] written, the
    windows read once and one slot of each written, count and head of both windows read and written, the inputs read, wf_env and
    status written"""
    lane = 8 * (2 * 4 + 2 * 16 + 2 + 3 + (ns + nl) + 2) + 4 * 4 * 2 + 8 * 3
    return 4 * lane + 8 * 3 + 8 * 6 + 4


def state_bytes(ns, nl):
    return 4 * (8 * (4 + 16 + 1 + ns + nl) + 4 * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="4096,16384,65536,262144", help="comma-separated batch sizes")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import bluerov2_amd as ba
    p = ba.RlsParams.default()
    bpu = bytes_per_update(p.n_short, p.n_long)
    runs = []
    for B in [int(b) for b in a.batch.split(",")]:
        rng = np.random.default_rng(0)
        r = ba.BatchRls(B)
        y = torch.tensor(rng.normal(size=(B, 4)), device="cuda"); acc = torch.tensor(rng.normal(size=(B, 4)), device="cuda")
        vel = torch.tensor(rng.normal(size=(B, 4)), device="cuda"); rpy = torch.tensor(rng.uniform(-0.3, 0.3, (B, 3)), device="cuda")
        ptrs = (y.data_ptr(), acc.data_ptr(), vel.data_ptr(), rpy.data_ptr())
        for _ in range(max(a.warmup, p.n_long)):    # the long window full: every later tick sums n_long entries
            r.update_device(*ptrs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r.update_device(*ptrs)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / a.steps
        ker = []
        for _ in range(10):
            r.update_device(*ptrs)
            ker.append(r.last_update_seconds())
        kt = float(np.median(ker))
        _, _, st = r.outputs()
        runs.append({"batch": B, "updates_per_s": B / kt, "us_per_launch": kt * 1e6, "wall_us_per_step": wall * 1e6,
                     "hbm_gbs": bpu * B / kt / 1e9, "hbm_frac": bpu * B / kt / 8e12, "state_mb": state_bytes(p.n_short, p.n_long) * B / 1e6,
                     "status_nonzero": int((st != 0).sum())})
        r.close()
        del y, acc, vel, rpy
    top = runs[-1]
    out = {"metric": "RLS-FF estimator updates/s (4 axes, windows 5 / 50)", "value": top["updates_per_s"], "unit": "updates/s",
           "batch": top["batch"], "steps": a.steps, "us_per_launch": top["us_per_launch"],
           "roofline_hbm": {"achieved": top["hbm_gbs"], "peak": 8000.0, "unit": "GB/s", "frac": top["hbm_frac"], "bytes_per_update": bpu},
           "batches": runs}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
