#!/usr/bin/env python3
"""The stand-off term of the fleet loop on one MI355X (brov_standoff_*).  Writes <out-dir>/standoff_bench.json and
<out-dir>/standoff_scenarios.txt.

Measurements, at V x C = 64 x 64 and 256 x 64, N = 20: the piers fixture moved so that one pier stands at the origin, the vehicles spread
round it on a circle of 10 m, circle candidates with distinct radii.
1. seconds of standoff_dist_kernel (brov_standoff_last_seconds: HIP events around the kernel) on the iterate the loops left, radius = reach;
2. the same at reach = +Inf; with both the node tests and triangle tests per query point (brov_standoff_eval_host's visits);
3. seconds of clearance_dist_kernel and of one solve of the batch, in the same run;
4. seconds per tick of brov_closed_loop_fleet (no logs: one host wait per run) with the term off and on, the two taking turns.
Median of `--repeats` after one warm-up each.

Scenario: four vehicles on a circle of 2 m at 0.5 m/s, each with a pillar of 0.5 m x 0.5 m across its reference 1.5 m ahead (three as
box_mesh triangles, one as a box of the scene), candidates of radius 2.0 ... 3.05 m.  For the term off, soft and hard: the smallest TRUE
distance of the flown states to the structure (tests/standoff_restatement.py's brute force over the logged states), and what the
vehicles did.  Two more runs put a post 0.3 m beside vehicle 0's start, inside the radius, under the hard weight: with first = 0 and with
first = 1."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N, TS = 20, 0.05


def median(v):
    return float(np.median(v))


def measure(a, ba, torch):
    tri = np.load(os.path.join(ROOT, "tests", "golden", "bridge2_piers.npz"))["tri"].astype(np.float64)
    tri = np.ascontiguousarray(tri + np.array([-19.47, 0.0, 11.5]))            # the pier at x = 17.7 ... 21.2 m, z = -36 ... -27 m to the origin, depth 20 m
    rows = []
    for V, C in [tuple(int(t) for t in sh.split("x")) for sh in a.shapes.split(",")]:
        B = V * C
        ang = 2.0 * np.pi * np.arange(V) / V
        xv = np.zeros((V, 12)); xv[:, 0] = -10.0 * np.cos(ang); xv[:, 1] = -10.0 * np.sin(ang); xv[:, 2] = -20.0; xv[:, 5] = ang - 0.5 * np.pi
        s = ba.BatchSolver(B, ba.SolverOptions(N, TS))
        s.set_params(ba.P_NOMINAL)
        s.set_candidate_params("circle", np.tile(9.0 + 2.0 * np.arange(C) / C, V), np.full(B, 0.5), np.repeat(ang, C))
        s.set_range_mesh(tri)
        info = s.range_mesh_info()
        f = ba.Fleet(s, C)

        def loop(on):
            s.init_iterate_default(); s.set_params(ba.P_NOMINAL); f.reset(); f.set_state(xv)
            if on:
                f.set_standoff(a.radius, a.weight, a.radius, 1)
            else:
                f.standoff_off()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            f.closed_loop(a.ticks, 0.0, TS, TS, 0.05, 1, log=False)
            return (time.perf_counter() - t0) / a.ticks

        loop(False); loop(True)
        off, on = [], []
        for _ in range(a.repeats):                                             # the two take turns
            off.append(loop(False)); on.append(loop(True))
        row = {"vehicles": V, "candidates": C, "batch": B, "triangles": int(info.triangles), "nodes": int(info.nodes), "leaf": int(info.leaf),
               "loop_off_seconds_per_tick": median(off), "loop_on_seconds_per_tick": median(on),
               "loop_off_min_max": [float(np.min(off)), float(np.max(off))], "loop_on_min_max": [float(np.min(on)), float(np.max(on))],
               "on_over_off": median(on) / median(off)}
        s.enable_timing(True)
        f.set_clearance(a.radius, a.weight, 1)
        points = B * N                                                         # stages 1 ... N
        for name, reach in (("reach_radius", a.radius), ("reach_inf", np.inf)):
            f.set_standoff(a.radius, a.weight, reach, 1)
            f.standoff_eval()
            secs = []
            for _ in range(a.repeats):
                f.standoff_eval()
                secs.append(f.standoff_seconds())
            s2, _, vis = f.standoff_eval(visits=True)
            nt, tt = float(vis[:, 0].sum()) / points, float(vis[:, 1].sum()) / points
            row[name] = {"reach": None if np.isinf(reach) else reach, "dist_kernel_seconds_median": median(secs), "dist_kernel_seconds_min": float(np.min(secs)),
                         "query_points": points, "node_tests_per_point": nt, "triangle_tests_per_point": tt,
                         "points_per_second": points / median(secs), "bytes_requested_per_tick": int(points * (24 + 64 * nt + 72 * tt)),
                         "candidates_inside_radius": int((s2 < a.radius ** 2).sum()), "candidates_below_reach": int((s2 < reach * reach).sum())}
        solve, clr = [], []
        for _ in range(a.repeats):
            s.solve(sync=True); solve.append(s.last_solve_seconds()[0])
            f.clearance_eval(); clr.append(f.clearance_seconds())
        row["solve_seconds_median"] = median(solve); row["clearance_dist_kernel_seconds_median"] = median(clr)
        row["dist_kernel_over_solve"] = row["reach_radius"]["dist_kernel_seconds_median"] / row["solve_seconds_median"]
        rows.append(row)
        f.close(); s.close()
    return {"metric": "stand-off term of the fleet loop: nearest-distance kernel against the bridge piers, and the loop with the term on and off",
            "N": N, "ticks": a.ticks, "repeats": a.repeats, "radius": a.radius, "weight": a.weight, "first": 1, "rows": rows}


def scenarios(a, ba):
    import standoff_restatement as SR
    from bluerov2_amd.mesh import box_mesh
    V, C, R, speed, half = 4, 8, 2.0, 0.5, 0.25
    ang = 0.5 * np.pi * np.arange(V)
    ahead = ang + 1.5 / R                                                      # 1.5 m of arc ahead of every vehicle
    cen = np.stack([-R * np.cos(ahead), -R * np.sin(ahead)], axis=1)
    lo = np.concatenate([cen - half, np.full((V, 1), -25.0)], axis=1); hi = np.concatenate([cen + half, np.full((V, 1), -15.0)], axis=1)
    tri = np.concatenate([box_mesh(lo[v], hi[v]) for v in range(V - 1)])
    st = SR.stored(np.concatenate([tri, box_mesh(lo[V - 1], hi[V - 1])]))      # the structure, all of it as triangles, for the true distance
    xv = np.zeros((V, 12)); xv[:, 0] = -R * np.cos(ang); xv[:, 1] = -R * np.sin(ang); xv[:, 2] = -20.0; xv[:, 5] = ang - 0.5 * np.pi; xv[:, 6] = speed
    lines = [f"The stand-off term in closed loop (python scripts/bench_standoff.py; brov_closed_loop_fleet, {a.scenario_ticks} ticks of {TS} s, N = {N}).",
             f"{V} vehicles on a circle of {R} m at {speed} m/s; a pillar of {2 * half} m x {2 * half} m across each reference 1.5 m ahead (three as box_mesh",
             f"triangles, one as a box of the scene); {C} candidates per vehicle, circles of radius 2.0 ... 3.05 m; radius {a.scenario_radius} m, reach "
             f"{a.scenario_reach} m, first 1.", "distance: the smallest true distance of the flown states (the logged x, every tick) to the structure, by brute force.", ""]
    # a post 0.3 m inside vehicle 0's start, for the last two runs: the vehicle BEGINS inside the radius
    post_lo, post_hi = np.array([[-1.7, -0.1, -25.0]]), np.array([[-1.5, 0.1, -15.0]])
    st_post = SR.stored(np.concatenate([tri, box_mesh(lo[V - 1], hi[V - 1]), box_mesh(post_lo[0], post_hi[0])]))
    for name, weight, first, post in (("off", None, 1, False), ("soft", a.scenario_soft, 1, False), ("hard", np.inf, 1, False),
                                      ("hard, first 0, a post 0.3 m beside vehicle 0's start", np.inf, 0, True),
                                      ("hard, first 1, the same post", np.inf, 1, True)):
        s = ba.BatchSolver(V * C, ba.SolverOptions(N, TS))
        s.set_params(ba.P_NOMINAL)
        s.set_candidate_params("circle", np.tile(R + 0.15 * np.arange(C), V), np.full(V * C, speed), np.repeat(ang, C))
        s.set_range_mesh(tri)
        s.set_range_scene(np.concatenate([lo[V - 1:], post_lo]) if post else lo[V - 1:], np.concatenate([hi[V - 1:], post_hi]) if post else hi[V - 1:])
        f = ba.Fleet(s, C)
        f.set_plant_params(np.tile(ba.P_NOMINAL, (V, 1)))
        f.set_state(xv)
        if weight is not None:
            f.set_standoff(a.scenario_radius, weight, a.scenario_reach, first)
        u, x, status, win = f.closed_loop(a.scenario_ticks, 0.0, TS, TS, 0.05, 1)
        d = np.sqrt(SR.point_min(x[:, :, :3].reshape(-1, 3), st_post if post else st)).reshape(x.shape[0], V)
        stats = f.standoff_stats()
        lines.append(f"term {name}" + ("" if weight is None else f" (weight {weight})"))
        for v in range(V):
            held = int((win[:, v] < 0).sum())
            tail = int(np.argmax(win[::-1, v] >= 0)) if (win[:, v] >= 0).any() else len(win)
            lines.append(f"  vehicle {v} ({'box' if v == V - 1 else 'mesh'}): smallest distance {d[:, v].min():.4f} m at tick {int(d[:, v].argmin())}, "
                         f"final distance {d[-1, v]:.4f} m; ticks without a winner (input held) {held}, of them at the end {tail}; "
                         f"winners used {sorted(set(int(w) for w in win[:, v]))}; arc flown {np.linalg.norm(np.diff(x[:, v, :2], axis=0), axis=1).sum():.3f} m; "
                         f"below {int(stats['below'][v])}, min_s2 {stats['min_s2'][v]:.4f}")
        lines.append("")
        f.close(); s.close()
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x64,256x64")
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--weight", type=float, default=100.0)
    ap.add_argument("--scenario-ticks", type=int, default=200)
    ap.add_argument("--scenario-radius", type=float, default=0.45)
    ap.add_argument("--scenario-reach", type=float, default=1.0)
    ap.add_argument("--scenario-soft", type=float, default=500.0)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--only", choices=["bench", "scenarios"], default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this script measures on a GPU"
    import bluerov2_amd as ba
    os.makedirs(a.out_dir, exist_ok=True)
    if a.only != "bench":
        txt = scenarios(a, ba)
        open(os.path.join(a.out_dir, "standoff_scenarios.txt"), "w").write(txt + "\n")
        print(txt)
    if a.only != "scenarios":
        res = measure(a, ba, torch)
        open(os.path.join(a.out_dir, "standoff_bench.json"), "w").write(json.dumps(res) + "\n")
        print(json.dumps(res))


if __name__ == "__main__":
    main()
