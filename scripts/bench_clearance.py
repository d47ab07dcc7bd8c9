#!/usr/bin/env python3
"""The inter-vehicle clearance term of the fleet loop on the device beside the same loop composed from Python (brov_clearance_*; DESIGN.md
section 4.12b).

At V x C = 64 x 64 and 256 x 64, N = 20, circle candidates with distinct radii per candidate, the vehicles spread along the circle:
1. seconds of clearance_dist_kernel (brov_clearance_last_seconds: HIP events around the kernel) beside the seconds of one solve of the batch;
2. planning ticks per second of brov_closed_loop_fleet with the term off (no logs: one host wait per run);
3. the same with the term on;
4. the same loop composed from Python the way it had to be before: solve -> get the iterate and the records -> d2min and re-scoring in numpy ->
   records up -> step(re-scored records) -> winners down -> numpy publish.  The numpy distance pass costs seconds per tick at these shapes, so
   this loop runs `--composed-ticks` ticks, `--composed-repeats` times.
All loops start from the same states and the same iterate.  Median of `--repeats` runs after one warm-up run each.  `--only off` measures
loop 2 alone (for a side-by-side with another build of the library).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_d2min(x, plan, V, C, shift, chunk=128):
    """clearance_restatement.d2min with candidates, peers and stages vectorised: the same operations per distance, in the same order"""
    N = plan.shape[1] - 1
    q = plan[:, np.minimum(np.arange(N + 1) + shift, N), :]
    out = np.empty(V * C)
    with np.errstate(invalid="ignore", over="ignore"):
        for b0 in range(0, V * C, chunk):
            p = x[b0:b0 + chunk, None, :, :3]
            dx, dy, dz = p[..., 0] - q[None, ..., 0], p[..., 1] - q[None, ..., 1], p[..., 2] - q[None, ..., 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            d2[np.isnan(d2)] = np.inf
            rows = np.arange(d2.shape[0])
            d2[rows, (b0 + rows) // C] = np.inf
            out[b0:b0 + chunk] = d2.reshape(d2.shape[0], -1).min(axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x64,256x64")
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--composed-ticks", type=int, default=4)
    ap.add_argument("--composed-repeats", type=int, default=2)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--weight", type=float, default=100.0)
    ap.add_argument("--only", choices=["off"], default=None)
    a = ap.parse_args()
    import torch
    import bluerov2_amd as ba
    N, TS, SHIFT, rows = 20, 0.05, 1, []
    if a.only is None:
        import clearance_restatement as CR
    for V, C in [tuple(int(t) for t in sh.split("x")) for sh in a.shapes.split(",")]:
        B = V * C
        radius = np.tile(2.0 + 0.5 * np.arange(C) / C, V)
        ang = 2.0 * np.pi * np.arange(V) / V                       # the vehicles spread along the circle they share
        xv = np.zeros((V, 12)); xv[:, 0] = -2.2 * np.cos(ang); xv[:, 1] = -2.2 * np.sin(ang); xv[:, 2] = -20.0; xv[:, 5] = ang - 0.5 * np.pi
        s = ba.BatchSolver(B, ba.SolverOptions(N, TS))
        s.set_params(ba.P_NOMINAL)
        s.set_candidate_params("circle", radius, np.full(B, 0.5), np.repeat(ang, C))
        f = ba.Fleet(s, C)

        def run(which):
            s.init_iterate_default(); s.set_params(ba.P_NOMINAL); f.reset(); f.set_state(xv)
            if which == "on":
                f.set_clearance(a.radius, a.weight, SHIFT)
            elif a.only is None:
                f.clearance_off()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            if which in ("off", "on"):
                f.closed_loop(a.ticks, 0.0, TS, TS, 0.05, 1, log=False)
                return (time.perf_counter() - t0) / a.ticks
            plan = np.repeat(xv[:, None, :3], N + 1, axis=1)
            for k in range(a.composed_ticks):
                s.set_yref_candidates_tick(0.0 + k * TS, TS); s.solve()
                xi, res = s.get_iterate()[0], s.results()
                d = host_d2min(xi, plan, V, C, SHIFT)
                inside = d < a.radius * a.radius
                res["cost"][inside] = res["cost"][inside] + a.weight * (a.radius * a.radius - d[inside])
                dev = torch.from_numpy(np.frombuffer(res.tobytes(), dtype=np.uint8).copy()).cuda()
                f.step(dev.data_ptr(), 0.05, 1)
                plan = CR.publish(plan, xi, f.last()[2], V, C, SHIFT)
            return (time.perf_counter() - t0) / a.composed_ticks

        row = {"vehicles": V, "candidates": C, "batch": B}
        for which in (("off",) if a.only else ("off", "on", "composed")):
            run(which)
            dts = [run(which) for _ in range(a.composed_repeats if which == "composed" else a.repeats)]
            row[which] = {"seconds_per_tick_median": float(np.median(dts)), "seconds_per_tick_min": float(np.min(dts)),
                          "seconds_per_tick_max": float(np.max(dts)), "ticks_per_s": 1.0 / float(np.median(dts))}
        if a.only is None:
            # the distance kernel and the solve of the same batch, alone, from the state the last loop left
            f.set_clearance(a.radius, a.weight, SHIFT)
            s.enable_timing(True)
            dist, solve = [], []
            for _ in range(a.repeats):
                s.solve(sync=True)
                solve.append(s.last_solve_seconds()[0])
                f.clearance_eval()
                dist.append(f.clearance_seconds())
            row["dist_kernel_seconds_median"] = float(np.median(dist)); row["dist_kernel_seconds_min"] = float(np.min(dist))
            row["solve_seconds_median"] = float(np.median(solve))
            row["dist_kernel_share_of_tick_on"] = row["dist_kernel_seconds_median"] / row["on"]["seconds_per_tick_median"]
            row["dist_kernel_over_solve"] = row["dist_kernel_seconds_median"] / row["solve_seconds_median"]
            row["on_over_composed_ticks_per_s"] = row["on"]["ticks_per_s"] / row["composed"]["ticks_per_s"]
            row["on_over_off_seconds_per_tick"] = row["on"]["seconds_per_tick_median"] / row["off"]["seconds_per_tick_median"]
            # per tick: V * C * (V - 1) * (N + 1) point distances of 8 flops (3 differences, 3 products, 2 sums) and a compare; the iterate's
            # positions are read as whole 96-byte stages (24 of them used), the plan once per group of 64 candidates through the scalar cache
            pairs = B * (V - 1) * (N + 1)
            row["point_distances_per_tick"] = pairs
            row["flops_per_tick"] = 8 * pairs
            row["dist_kernel_gflops"] = 8 * pairs / row["dist_kernel_seconds_median"] / 1e9
            row["iterate_bytes_touched_per_tick"] = B * (N + 1) * 96
            row["plan_bytes_per_tick_scalar_cache"] = ((B + 63) // 64) * V * (N + 1) * 24
            row["host_bytes_per_tick_composed"] = B * (N + 1) * 96 + 2 * 104 * B
        rows.append(row)
        f.close(); s.close()
    print(json.dumps({"metric": "fleet planning loop with the clearance term on the device against the loop composed from Python", "N": N,
                      "ticks": a.ticks, "repeats": a.repeats, "composed_ticks": a.composed_ticks, "composed_repeats": a.composed_repeats,
                      "radius": a.radius, "weight": a.weight, "shift": SHIFT, "rows": rows}))


if __name__ == "__main__":
    main()
