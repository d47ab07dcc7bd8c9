#!/usr/bin/env python3
"""make_dispatch_golden.py -- what the HOST decides for a solver, row by row, written to tests/golden/dispatch_table.json.

Every row sits on a boundary of a dispatch rule (horizons 4 | 11/12 | 23/24 | 47/48 | 80/81/82 | 128/129, batches around one and two
instances per CU, the three kernel_path values, uniform / general grid, rti_phase 0 and 1 -> 2, the tick mailbox limit, brov_solve_ticks,
the workspace-sizing development knobs).  Per row: create the solver, run the row's call(s) from the create-time iterate, record
device_bytes (every workspace-sizing decision), window_stages, lds_kernel_info, last_kernel_path, how many instances the parallel-in-time
kernel completed, the status vector and -- for rti_phase rows -- the return code and error text of each call.

Run ONCE on the MI355X at the commit whose decisions are the reference (the parent of a change to the dispatch code):
    python scripts/make_dispatch_golden.py [--out FILE]   # writes tests/golden/dispatch_table.json (or FILE)
    python scripts/make_dispatch_golden.py --check [--out FILE]   # walks the table again and compares with the file
    python scripts/make_dispatch_golden.py --walk     # walks the table and writes nothing (a profiler's workload)
tests/test_gpu_dispatch.py recomputes the rows and requires equality on every field."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_table.json")

AUTO, STREAMING, FUSED = 0, 1, 2
HORIZONS = (4, 11, 12, 23, 24, 47, 48, 80, 81, 82, 128, 129)


def rows():
    """(N, B as a formula in the CU count, kernel_path, general grid, call, environment) -- call: "solve" | "phase12" (rti_phase 1 then 2) |
    "phase2" (no preparation) | "phase1-grid-2" (a setter between the two) | "tick" | "ticks" (brov_solve_ticks, two steps)"""
    t = []
    add = lambda N, B, path=AUTO, grid=False, call="solve", **env: t.append(dict(N=N, B=B, path=path, grid=grid, call=call, env=env))  # noqa: E731
    for N in HORIZONS:                                   # every horizon on either side of one instance per CU
        add(N, "1"); add(N, "cus+1")
    for N, B in ((47, "2*cus"), (48, "cus"), (48, "2*cus"), (48, "2*cus+1"), (80, "cus"), (80, "2*cus"), (80, "2*cus+1"), (81, "cus")):
        add(N, B)                                        # resident mode / parallel-in-time rounds: their batch limits at their horizon limits
    for N, B, path in ((12, "1", STREAMING), (48, "1", STREAMING), (23, "1", FUSED), (24, "1", FUSED), (129, "cus+1", FUSED)):
        add(N, B, path)
    for N, B in ((11, "1"), (23, "1"), (24, "1"), (24, "cus+1"), (48, "cus+1"), (80, "1"), (129, "1")):
        add(N, B, grid=True)
    for N, B in ((4, "1"), (11, "1"), (23, "cus"), (23, "cus+1"), (24, "1"), (48, "cus+1"), (80, "cus"), (81, "1"), (82, "1")):
        add(N, B, call="phase12")
    add(24, "1", grid=True, call="phase12")
    add(24, "1", path=STREAMING, call="phase12")
    add(24, "1", call="phase2")
    add(24, "1", call="phase1-grid-2")
    add(12, "1", call="phase1-grid-2")
    for N, B in ((11, "1"), (12, "1"), (12, "64"), (12, "65"), (24, "1"), (24, "65")):
        add(N, B, call="tick")                           # the mailbox limit (64 instances); N = 11: two waves, no mailbox variant
    for N, B in ((11, "2"), (12, "2"), (24, "1"), (24, "cus+1"), (48, "cus+1"), (129, "cus+1")):
        add(N, B, call="ticks")
    add(12, "2", grid=True, call="ticks")
    add(48, "1", BROV_DEV_NO_RESIDENT="1"); add(48, "cus+1", BROV_DEV_NO_RESIDENT="1"); add(24, "1", call="phase12", BROV_DEV_NO_RESIDENT="1")
    add(48, "cus+1", BROV_PIT_ROUNDS="0"); add(80, "2*cus", BROV_PIT_ROUNDS="0")
    add(12, "1", BROV_DEV_FORCE_WINDOWED="1"); add(12, "cus+1", BROV_DEV_FORCE_WINDOWED="1")
    add(12, "1", call="phase12", BROV_DEV_FORCE_WINDOWED="1"); add(12, "2", call="ticks", BROV_DEV_FORCE_WINDOWED="1")
    add(23, "1", call="phase12", BROV_SPLIT_RESIDENT="0"); add(24, "1", call="phase12", BROV_SPLIT_RESIDENT="0")
    return t


def inputs(B, N):
    """deterministic inputs: a hover reference at the create-time depth, instances spread around it, every 16th far enough off to saturate"""
    b = np.arange(B)
    x0 = np.zeros((B, 12))
    x0[:, 0] = 0.1 * ((b % 7) - 3); x0[:, 1] = 0.05 * ((b % 5) - 2); x0[:, 2] = -20.0 + 0.1 * (b % 3)
    x0[b % 16 == 0, :3] += np.array([4.0, -4.0, 3.0])
    yref = np.zeros((N + 1, 16)); yref[:, 2] = -20.0
    return x0, yref


def run_row(ba, row, cus):
    N, B = row["N"], int(eval(row["B"], {"cus": cus}))
    keep = {k: os.environ.get(k) for k in row["env"]}
    os.environ.update(row["env"])
    try:
        s = ba.BatchSolver(B, ba.SolverOptions(N, 1.0 / N, kernel_path=row["path"]), device=0)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    out = dict(device_bytes=s.device_bytes, window_stages=s.window_stages())
    x0, yref = inputs(B, N)
    s.set_x0(x0); s.set_yref(yref); s.set_params(ba.P_NOMINAL)
    ts = (1.0 / N) * (1.0 + 0.1 * (np.arange(N) % 2))
    if row["grid"]:
        s.set_time_steps(ts)
    calls, path = [], []

    def do_phase(p):
        rc = int(s._L.brov_solve_phase(s._h, C.c_void_p(0), p))
        calls.append([p, rc, s._L.brov_last_error().decode() if rc else ""])
        if rc == 0:
            path.append(s.last_kernel_path())
    call = row["call"]
    if call == "solve":
        s.solve(sync=True)
    elif call == "phase12":
        do_phase(1); do_phase(2)
    elif call == "phase2":
        do_phase(2)
    elif call == "phase1-grid-2":
        do_phase(1); s.set_time_steps(ts); do_phase(2)
    elif call == "tick":
        s.tick(x0=x0, yref=yref)
    elif call == "ticks":
        s.solve_ticks(2, 0, sync=True)
    out.update(lds_kernel_info=s.lds_kernel_info(), last_kernel_path=s.last_kernel_path(), pit_done=int(s.pit_last().sum()),
               status=s.results()["status"].tolist())
    if calls:
        out.update(phase_calls=calls, phase_paths=path)
    s.close()
    return out


def walk():
    import torch
    import bluerov2_amd as ba
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    return dict(cus=cus, rows=[dict(row, result=run_row(ba, row, cus)) for row in rows()])


def differences(want, got):
    """human-readable list of the fields in which two walks differ"""
    if want["cus"] != got["cus"]:
        return [f"CU count {want['cus']} != {got['cus']}"]
    out = []
    if len(want["rows"]) != len(got["rows"]):
        out.append(f"{len(want['rows'])} rows != {len(got['rows'])}")
    for a, b in zip(want["rows"], got["rows"]):
        key = {k: a[k] for k in ("N", "B", "path", "grid", "call", "env")}
        if key != {k: b[k] for k in key}:
            out.append(f"row definition differs: {key}")
            continue
        for f in sorted(set(a["result"]) | set(b["result"])):
            if a["result"].get(f) != b["result"].get(f):
                out.append(f"{key}: {f}: expected {a['result'].get(f)!r}, got {b['result'].get(f)!r}")
    return out


if __name__ == "__main__":
    table = json.loads(json.dumps(walk()))   # (through JSON: tuples and lists compare equal afterwards)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    if "--walk" in sys.argv:
        print(f"walked {len(table['rows'])} rows on {table['cus']} CUs")
    elif "--check" in sys.argv:
        with open(out) as f:
            diff = differences(json.load(f), table)
        print("\n".join(diff) if diff else f"{len(table['rows'])} rows equal to {out}")
        sys.exit(1 if diff else 0)
    else:
        with open(out, "w") as f:
            f.write('{"cus": %d, "rows": [\n%s\n]}\n' % (table["cus"], ",\n".join(json.dumps(r) for r in table["rows"])))
        print(f"wrote {len(table['rows'])} rows to {out}")
