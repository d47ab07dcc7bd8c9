#!/usr/bin/env python3
"""The bridge-pier inspection mission flown on the CPU against the reference's own bridge: the restated controller
(tests/inspect_restatement.py) and the restated range stage against a triangle mesh (tests/mesh_restatement.py, brute force) in a loop with
the oracle plant (oracle/bluerov2_oracle.c, one RK4 step per tick), from the bridge demo's launch pose against the underwater part of
bridge2.STL (tests/golden/bridge2_piers.npz).  scripts/inspect_cpu_scenarios.py flies the same loop against one box and never completes the
mission: it comes round a box corner at 0.7 m and stays in the node's "state machine failed" branch.  This script asks the same of the
geometry the demo really spawns, under the two flag settings DESIGN.md section 4.9i reports (both of the node's quirks on; per-loop PID
accumulators), and reports rounds, the failed branch's first tick and the range there, and whether the mission completes; it asserts
nothing.  Writes profiles/inspect_mesh_scenarios.txt (--out)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def fly(orc, tri, flags, ticks):
    import inspect_restatement as R
    import mesh_restatement as M
    from bluerov2_amd import P_NOMINAL
    from bluerov2_amd import inspect as I
    par, cam = I.default_inspect_params(), I.default_range_params()
    par.flags = flags
    st = M.stored(tri)
    s, t = I.initial_state(par, 1), I.initial_stats(1)
    x = np.zeros(12)
    x[:3], x[5] = I.START_POSE[:3], I.START_POSE[3]
    status, rng_log, x_log, first_failed = [], [], [x.copy()], None
    for k in range(ticks):
        rng, hits, _ = M.cast(R.rot_np(*x[3:6]), x[:3], cam, st)
        rec, failed = R.control(par, s[0], t[0], rng, x[2], x[5])
        if failed and first_failed is None:
            first_failed = (k, rng, hits)
        x = orc.rk4(x, rec["u0"], P_NOMINAL, par.dt)
        status.append(int(s[0]["status"])); rng_log.append(rng); x_log.append(x.copy())
        if not np.all(np.isfinite(x)) or abs(x[2]) > 500.0:
            break
    return (par, s[0], t[0], np.array(status), np.array(rng_log), np.array(x_log)), first_failed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inspect_mesh_scenarios.txt"))
    args = ap.parse_args()
    from inspect_cpu_scenarios import report
    from oracle.oracle_ffi import Oracle, build
    build()
    orc = Oracle()
    tri = np.load(os.path.join(ROOT, "tests", "golden", "bridge2_piers.npz"))["tri"]
    lines = ["Bridge-pier inspection mission on the CPU loop against the reference's bridge (scripts/inspect_mesh_cpu_scenarios.py): restated controller,",
             f"restated range stage against the {len(tri)} triangles of bridge2.STL with a vertex below z = -5 (brute force), oracle plant, launch pose",
             "(17.97842, 3.259887, -34.5, yaw pi/2); a report, not a test.", ""]
    for name, flags in (("both quirks on (the node)", 3), ("shared PID off", 2)):
        run, first = fly(orc, tri, flags, args.ticks)
        t = run[2]
        lines += report(name, *run)
        if first is None:
            lines.append("   the 'state machine failed' branch was never entered")
        else:
            lines.append(f"   'state machine failed' first entered at tick {first[0]} with range {first[1]:.4f} m ({first[2]} of 1600 rays returned)")
        lines.append(f"   rounds: {int(t['rounds'])}   mission completes: {'yes, at tick %d' % int(t['first_done']) if int(t['first_done']) >= 0 else 'no'}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
