#!/usr/bin/env python3
"""Cost of the plant's thrust-curve stage (brov_curve_*).

1. At B = 16 384 and 262 144, for each of LINEAR, BASIC, TABLE at K = 201 (the T200 fixture, amps column included) and TABLE with a pre table
   (the fixture's inverse), on the same run: the plant step with every stage off (plant_kernel alone), with the curve stage alone (one BOTH
   launch ahead of it), with the rotor stage alone (rotor_shift_kernel ahead of it; tau = 0.2 s: the yardstick) and with both (COMMAND, rotor
   shift, THRUST), and one launch of BOTH, COMMAND, THRUST and of the rotor shift by the library's own HIP events (brov_curve_last_seconds,
   brov_rotor_last_seconds: the launches of the last plant step).  `--steps` plant steps enqueued back to back between two HIP events, no host
   wait in between; the forms take turns inside every repeat, so that a drift of the machine meets all of them; median of `--repeats` trains
   after one warm-up round, microseconds per step.
2. brov_closed_loop_dob, 64 ticks at B = 4096, N = 20, with the stage on (T200 table, inverse pre table, 4 us steps, behind rotors of
   tau = 0.2 s, the observer fed the delivered thrusts) and with the rotors alone, taking turns: ms per tick.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KGF_TO_THRUST, PWM_PER_THRUST = 60.0, 0.2     # units for the tables: 250 thrust units of the record are 50 us, 1 kgf is 60 of them


def t200(ba):
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "t200_16v.json")))
    return ba.curve_from_pwm_table(d["pwm"], d["kgf"], d["amps"])


def configure(s, ba, mode, tab, **kw):
    x, y, a = tab
    if mode == "linear":
        s.set_thrust_curve(**kw)
    elif mode == "basic":
        s.set_thrust_curve(kind="basic", k=1.0 / 250.0, **kw)
    elif mode == "table":
        s.thrust_curve_table("curve", x, y, a)
        s.set_thrust_curve(kind="table", pre="poly", pre_poly=(0.0, 0.0, 0.0, PWM_PER_THRUST, 0.0), quantum=4.0, eff=KGF_TO_THRUST, **kw)
    else:
        ix, iy = ba.inverse_table(x, y * KGF_TO_THRUST)
        s.thrust_curve_table("curve", x, y, a); s.thrust_curve_table("pre", ix, iy)
        s.set_thrust_curve(kind="table", pre="table", quantum=4.0, eff=KGF_TO_THRUST, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="16384,262144")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--loop-batch", type=int, default=4096)
    ap.add_argument("--loop-ticks", type=int, default=64)
    a = ap.parse_args()
    import torch
    import bluerov2_amd as ba
    from bench import synthetic_inputs
    N = 20
    h = 0.05 / a.steps                          # a short step: the state stays where it is over the train
    tab = t200(ba)
    kernels = []
    for B in [int(b) for b in a.batch.split(",")]:
        x0, circ = synthetic_inputs(B, seed=3, noise=False)
        s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1))); s.set_yref(circ[:N + 1])
        s.solve(sync=True)                      # an input for the plant to hold
        for mode in ("linear", "basic", "table", "table_pre"):
            forms = ("off", "curve", "rotor", "curve_rotor")
            us = {f: [] for f in forms}
            single = {"both": [], "command": [], "thrust": [], "rotor_shift": []}
            for rep in range(a.repeats + 1):
                for form in forms:
                    s.rotor_off(); s.thrust_curve_off()
                    if "rotor" in form:
                        s.set_rotors(0.2, h=h)
                    if "curve" in form:
                        configure(s, ba, mode, tab)
                    s.set_x0(x0)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        s.plant_step(h, 1)
                    e1.record(); torch.cuda.synchronize()
                    if rep:                                   # the first round warms up
                        us[form].append(e0.elapsed_time(e1) * 1e3 / a.steps)
                        if form == "curve":
                            single["both"].append(s.thrust_curve_last_seconds()[1] * 1e6)
                        elif form == "rotor":
                            single["rotor_shift"].append(s.rotor_last_seconds() * 1e6)
                        elif form == "curve_rotor":
                            c, t = s.thrust_curve_last_seconds()
                            single["command"].append(c * 1e6); single["thrust"].append(t * 1e6)
            row = {"batch": B, "mode": mode}
            for form in forms:
                row[form] = {"us_per_step_median": float(np.median(us[form])), "us_per_step_min": float(np.min(us[form])),
                             "us_per_step_max": float(np.max(us[form]))}
            for name, v in single.items():
                row[name + "_us_last_launch"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
            row["both_over_rotor_shift"] = row["both_us_last_launch"]["median"] / row["rotor_shift_us_last_launch"]["median"]
            kernels.append(row)
        s.close()
    # ---- the DOB loop behind rotors with the stage on and off ----------------------------------------------------------------------
    B, K = a.loop_batch, a.loop_ticks
    x0, circ = synthetic_inputs(B, seed=2, noise=False)
    ep = ba.EkfParams.default(); ep.compensate_coef = 1.0; ep.rotor_constant = 1.0
    for j in range(12, 24):
        ep.K[j] = 0.0
    loops = {}
    solvers = {}
    for name in ("off", "on"):
        s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1))); s.set_trajectory(circ)
        s.set_rotors(0.2, observer_applied=True)
        if name == "on":
            configure(s, ba, "table_pre", tab, observer_applied=True)
        e = ba.BatchEkf(B, ep)
        s.closed_loop_dob(e, ticks=5, line0=0, log=False)
        solvers[name] = (s, e, [])
    for rep in range(3):                                   # the two take turns
        for name, (s, e, dts) in solvers.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            s.closed_loop_dob(e, ticks=K, line0=5 + rep * K, log=False)
            dts.append((time.perf_counter() - t0) / K)
    for name, (s, e, dts) in solvers.items():
        dt = float(np.median(dts))
        loops[name] = {"ticks_per_s": B / dt, "ms_per_tick": dt * 1e3, "ms_per_tick_all": [d * 1e3 for d in dts],
                       "status_nonzero": int((s.results()["status"] != 0).sum())}
        e.close(); s.close()
    loops["on_over_off_ms_per_tick"] = loops["on"]["ms_per_tick"] / loops["off"]["ms_per_tick"]
    print(json.dumps({"metric": "plant step behind the thrust-curve stage (one BOTH launch), behind the rotor stage, behind both (COMMAND, rotor "
                                "shift, THRUST) and with neither, us per step; one BOTH, COMMAND, THRUST and rotor shift launch, us; DOB loop "
                                "behind rotors with the curve stage on and off, ms per tick", "steps": a.steps, "repeats": a.repeats,
                      "kernels": kernels, "dob_loop": {"batch": B, "N": N, "ticks": K, **loops}}))


if __name__ == "__main__":
    main()
