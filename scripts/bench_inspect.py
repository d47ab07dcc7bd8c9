#!/usr/bin/env python3
"""The inspection loop timed on one GPU:
  * the tick kernel (inspect_tick_kernel: roi * roi rays per instance against K boxes, then the controller in lane 0) at B = 4096, 16 384 and
    262 144 with roi = 40, for K = 1 and K = 8: HIP events around the launch, median of 10, three repeated medians whose spread is reported;
  * the FP64 operations the rays execute per ray-box pair (6 differences, 6 products, 6 min and 6 max = 24; the three compares and the
    per-ray part -- two quotients, the direction, three reciprocals, the range factor -- are left out of the count) over that time, as a
    fraction of the FP64 vector peak: 78.6 TFLOP/s, half the FP32 vector peak of the microarchitecture guide, a peak that counts a fused
    multiply-add as two, which a kernel that must round every operation on its own cannot issue: half of it is the most it could reach;
  * brov_closed_loop_inspect per tick at B = 4096 (wall clock around the call, which ends in its host wait) beside the same calls composed
    from Python.
There is no threshold: the capability has no parent to compare against.  Prints one JSON line; --out FILE also writes it there
(profiles/inspect_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VECTOR_PEAK = 78.6e12
OPS_PER_PAIR = 24


def boxes(K):
    """the pier, and K - 1 boxes behind it that every ray tests and none hits first"""
    from bluerov2_amd import inspect as I
    lo, hi = [list(I.PIER_LO)], [list(I.PIER_HI)]
    for k in range(1, K):
        lo.append([I.PIER_LO[0], I.PIER_HI[1] + 2.0 * k, I.PIER_LO[2]])
        hi.append([I.PIER_HI[0], I.PIER_HI[1] + 2.0 * k + 1.0, I.PIER_HI[2]])
    return np.array(lo), np.array(hi)


def solver(ba, B, K, N=20, dt=0.05):
    from bluerov2_amd import inspect as I
    s = ba.BatchSolver(B, ba.SolverOptions(N, dt), device=0)
    rng = np.random.default_rng(0)
    x0 = np.zeros((B, 12))
    x0[:, :3], x0[:, 5] = I.START_POSE[:3], I.START_POSE[3]
    x0[:, 0] += rng.uniform(0.0, 2.5, B); x0[:, 1] += rng.uniform(-0.3, 0.3, B); x0[:, 3:6] += rng.normal(size=(B, 3)) * 0.02
    s.set_x0(x0); s.set_params(ba.P_NOMINAL)
    s.set_range_scene(*boxes(K))
    s.set_range(sigma=0.01, seed=1)
    s.set_inspect()
    return s


def tick_kernel(ba, B, K, roi=40):
    s = solver(ba, B, K)
    for _ in range(3):
        s.inspect_step()
    med = []
    for _ in range(3):
        t = []
        for _ in range(10):
            s.inspect_step()
            t.append(s.inspect_last_seconds())
        med.append(float(np.median(t)))
    hits = s.range_eval(0, s.get_x0())["hits"]
    s.close()
    t = float(np.median(med))
    pairs = B * roi * roi * K
    return {"batch": B, "boxes": K, "roi": roi, "tick_us": t * 1e6, "tick_us_medians": [m * 1e6 for m in med], "spread_us": (max(med) - min(med)) * 1e6,
            "ray_box_pairs": pairs, "pairs_per_second": pairs / t, "fp64_ops_per_pair": OPS_PER_PAIR, "fp64_tflops": OPS_PER_PAIR * pairs / t / 1e12,
            "fraction_of_fp64_vector_peak": OPS_PER_PAIR * pairs / t / FP64_VECTOR_PEAK, "mean_hits": float(hits.mean())}


def loop(ba, B=4096, ticks=200, dt=0.05):
    a, b = solver(ba, B, 1), solver(ba, B, 1)
    a.closed_loop_inspect(20, dt, 1, log=False)
    for _ in range(20):
        b.inspect_step(); b.plant_step(dt, 1)
    b._chk(b._L.brov_synchronize(b._h, None), "synchronize")
    reps = []
    for _ in range(3):
        t0 = time.perf_counter()
        a.closed_loop_inspect(ticks, dt, 1, log=False)
        t1 = time.perf_counter()
        for _ in range(ticks):
            b.inspect_step(); b.plant_step(dt, 1)
        b._chk(b._L.brov_synchronize(b._h, None), "synchronize")
        t2 = time.perf_counter()
        reps.append(((t1 - t0) / ticks, (t2 - t1) / ticks))
    same = a.get_x0().tobytes() == b.get_x0().tobytes()
    a.close(); b.close()
    lo, co = float(np.median([r[0] for r in reps])), float(np.median([r[1] for r in reps]))
    return {"batch": B, "ticks": ticks, "closed_loop_inspect_us_per_tick": lo * 1e6, "composed_us_per_tick": co * 1e6,
            "closed_loop_inspect_ticks_per_second": 1.0 / lo, "composed_ticks_per_second": 1.0 / co, "instance_ticks_per_second": B / lo,
            "same_final_state": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batches", type=int, nargs="*", default=[4096, 16384, 262144])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_inspect.py needs a GPU: nothing here can be measured without one")
    import bluerov2_amd as ba
    res = {"metric": "inspection tick kernel, roi 40 (time per launch)", "fp64_vector_peak_tflops": FP64_VECTOR_PEAK / 1e12,
           "tick": [tick_kernel(ba, B, K) for B in args.batches for K in (1, 8)], "loop": loop(ba)}
    big = [r for r in res["tick"] if r["boxes"] == 8][-1]
    res["value"], res["unit"] = big["fraction_of_fp64_vector_peak"], "fraction of the FP64 vector peak (largest batch, 8 boxes)"
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
