#!/usr/bin/env python3
"""The bridge-pier inspection mission flown on the CPU: the restated range stage and controller (tests/inspect_restatement.py) in a loop with
the oracle plant (oracle/bluerov2_oracle.c, one RK4 step per tick), from the bridge demo's launch pose against its pier.  Nobody has run this
mission outside Gazebo: the script reports what happens -- ticks per side and per round, the statuses visited, whether the "state machine
failed" branch is ever entered, the stand-off RMS -- with both of the node's quirks on, and with each of them off; it asserts nothing.
Writes profiles/inspect_scenarios.txt (--out)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fly(orc, flags, ticks, sigma=0.0, seed=0):
    import inspect_restatement as R
    from bluerov2_amd import P_NOMINAL
    from bluerov2_amd import inspect as I
    par, cam = I.default_inspect_params(), I.default_range_params()
    par.flags, cam.seed = flags, seed
    s, t = I.initial_state(par, 1), I.initial_stats(1)
    x = np.zeros(12)
    x[:3], x[5] = I.START_POSE[:3], I.START_POSE[3]
    status, rng_log, x_log = [], [], [x.copy()]
    for k in range(ticks):
        rot = R.rot_np(*x[3:6])
        rng = R.range_eval(rot[None, :], x[None, :], cam, [I.PIER_LO], [I.PIER_HI], sigma=sigma, m=k)["range"][0]
        rec, _ = R.control(par, s[0], t[0], rng, x[2], x[5])
        x = orc.rk4(x, rec["u0"], P_NOMINAL, par.dt)
        status.append(int(s[0]["status"])); rng_log.append(rng); x_log.append(x.copy())
        if not np.all(np.isfinite(x)) or abs(x[2]) > 500.0:
            break
    return par, s[0], t[0], np.array(status), np.array(rng_log), np.array(x_log)


def report(name, par, s, t, status, rng, x):
    out = [f"== {name}: {len(status)} ticks of {par.dt} s"]
    out.append(f"   ticks in status 0..5: {list(map(int, t['ticks']))}   statuses visited: {sorted(set(status.tolist()))}")
    out.append(f"   'state machine failed' branch entered: {int(t['failed'])} time(s)   rounds: {int(t['rounds'])}   "
               f"mission completed at tick: {int(t['first_done'])}")
    n0 = int(t["ticks"][0])
    rms = float(np.sqrt(t["standoff_sq"] / n0)) if n0 else float("nan")
    out.append(f"   stand-off RMS over the status-0 ticks: {rms:.4f} m   smallest non-zero range: {float(t['min_range']):.4f} m")
    # the sides: runs of ticks between two turns (a turn begins where status 2 follows another status)
    turns = [k for k in range(1, len(status)) if status[k] == 2 and status[k - 1] != 2]
    sides = np.diff([0] + turns).tolist()
    out.append(f"   turns begun at ticks {turns[:12]}{' ...' if len(turns) > 12 else ''}   ticks per side: {sides[:12]}")
    if len(turns) >= 4:
        out.append(f"   ticks per round (four sides): {[int(turns[i + 3] - (turns[i - 1] if i else 0)) for i in range(0, len(turns) - 3, 4)]}")
    out.append(f"   final pose: x {x[-1, 0]:.3f} y {x[-1, 1]:.3f} z {x[-1, 2]:.3f} yaw {x[-1, 5]:.3f}   yaw_sum {float(s['yaw_sum']):.3f} "
               f"ref_yaw {float(s['ref_yaw']):.3f} ref_z {float(s['ref_z']):.3f}")
    out.append(f"   largest |roll|, |pitch|: {np.abs(x[:, 3]).max():.3f}, {np.abs(x[:, 4]).max():.3f} rad   "
               f"largest speed: {np.linalg.norm(x[:, 6:9], axis=1).max():.3f} m/s")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inspect_scenarios.txt"))
    args = ap.parse_args()
    from oracle.oracle_ffi import Oracle, build
    build()
    orc = Oracle()
    lines = ["Bridge-pier inspection mission on the CPU loop (scripts/inspect_cpu_scenarios.py): restated range stage and controller, oracle plant,",
             "launch pose (17.97842, 3.259887, -34.5, yaw pi/2) against the pier (17.74002, 5.259887) ... (21.34002, 8.97006); a report, not a test.", ""]
    for name, flags, sigma in (("both quirks on (the node)", 3, 0.0), ("shared PID off", 2, 0.0), ("float yaw off", 1, 0.0), ("both off", 0, 0.0),
                               ("both on, range noise sigma 0.01 m", 3, 0.01)):
        lines += report(name, *fly(orc, flags, args.ticks, sigma)) + [""]
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
