#!/usr/bin/env python3
"""The inspection tick against a triangle mesh timed on one GPU, in the manner of scripts/bench_inspect.py:
  * the mesh tick kernel (inspect_mesh_tick_kernel: roi * roi rays per instance through the skip-link hierarchy, then the controller in
    lane 0) at B = 4096 and 16 384 with roi = 40, on the piers of the reference's bridge (tests/golden/bridge2_piers.npz, 496 triangles) and
    on a procedural icosphere of 81 920 triangles seen from inside: HIP events around the launch, median of 10, three repeated medians whose
    spread is reported;
  * the box tick kernel (inspect_tick_kernel) with K = 8 boxes in the same run, for scale;
  * the node tests and triangle tests per ray of the same states (brov_mesh_eval_host's visits).
There is no threshold: the capability has no parent to compare against.  Prints one JSON line; --out FILE also writes it there
(profiles/mesh_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
ROI = 40


def solver(ba, B, x0, N=20, dt=0.05):
    s = ba.BatchSolver(B, ba.SolverOptions(N, dt), device=0)
    s.set_x0(x0); s.set_params(ba.P_NOMINAL)
    s.set_range(sigma=0.01, seed=1)
    return s


def pier_states(B):
    from bluerov2_amd import inspect as I
    rng = np.random.default_rng(0)
    x0 = np.zeros((B, 12))
    x0[:, :3], x0[:, 5] = I.START_POSE[:3], I.START_POSE[3]
    x0[:, 0] += rng.uniform(0.0, 2.5, B); x0[:, 1] += rng.uniform(-0.3, 0.3, B); x0[:, 3:6] += rng.normal(size=(B, 3)) * 0.02
    return x0


def sphere_states(B, radius):
    rng = np.random.default_rng(1)
    x0 = np.zeros((B, 12))
    x0[:, :3] = rng.uniform(-0.4, 0.4, (B, 3)) * radius
    x0[:, 3:6] = rng.uniform(-1.0, 1.0, (B, 3)) * [0.5, 0.5, np.pi]
    return x0


def timed_ticks(s):
    for _ in range(3):
        s.inspect_step()
    med = []
    for _ in range(3):
        t = []
        for _ in range(10):
            s.inspect_step()
            t.append(s.inspect_last_seconds())
        med.append(float(np.median(t)))
    return float(np.median(med)), med


def mesh_tick(ba, B, name, tri, x0):
    s = solver(ba, B, x0)
    s.set_range_mesh(tri)
    s.set_inspect()
    info = s.range_mesh_info()
    t, med = timed_ticks(s)
    o = s.range_eval(0, x0, visits=True)
    s.close()
    rays = B * ROI * ROI
    return {"mesh": name, "batch": B, "roi": ROI, "triangles": int(info.triangles), "nodes": int(info.nodes), "depth": int(info.depth), "leaf": int(info.leaf),
            "device_bytes": int(info.device_bytes), "tick_us": t * 1e6, "tick_us_medians": [m * 1e6 for m in med], "spread_us": (max(med) - min(med)) * 1e6,
            "rays_per_second": rays / t, "node_tests_per_ray": float(o["visits"][:, 0].sum() / rays), "triangle_tests_per_ray": float(o["visits"][:, 1].sum() / rays),
            "mean_hits": float(o["hits"].mean())}


def box_tick(ba, B, K=8):
    from bench_inspect import boxes
    s = solver(ba, B, pier_states(B))
    s.set_range_scene(*boxes(K))
    s.set_inspect()
    t, med = timed_ticks(s)
    s.close()
    return {"batch": B, "boxes": K, "roi": ROI, "tick_us": t * 1e6, "tick_us_medians": [m * 1e6 for m in med], "spread_us": (max(med) - min(med)) * 1e6,
            "rays_per_second": B * ROI * ROI / t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batches", type=int, nargs="*", default=[4096, 16384])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py needs a GPU: nothing here can be measured without one")
    import bluerov2_amd as ba
    from bluerov2_amd.mesh import icosphere
    piers = np.load(os.path.join(ROOT, "tests", "golden", "bridge2_piers.npz"))["tri"]
    sphere = icosphere(6, 10.0)
    assert len(sphere) == 81920
    res = {"metric": "inspection tick kernel against a mesh, roi 40 (time per launch)", "mesh_tick": [], "box_tick": []}
    for B in args.batches:
        res["mesh_tick"].append(mesh_tick(ba, B, "bridge2 piers", piers, pier_states(B)))
        res["mesh_tick"].append(mesh_tick(ba, B, "icosphere", sphere, sphere_states(B, 10.0)))
        res["box_tick"].append(box_tick(ba, B))
    big = [r for r in res["mesh_tick"] if r["mesh"] == "icosphere"][-1]
    res["value"], res["unit"] = big["rays_per_second"], "rays per second (largest batch, 81 920 triangles)"
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
