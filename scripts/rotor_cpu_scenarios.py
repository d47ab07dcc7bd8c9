#!/usr/bin/env python3
"""The rotor-lag scenarios of DESIGN.md section 4.9f on the CPU loop (tests/rotor_restatement.py: the oracle's RTI step, the restated rotor
stage, the oracle's model as plant): N = 20, B = 4, seed 21, the circle, Ts = 0.05, the setup of scripts/delay_cpu_scenarios.py.  Needs no
GPU (the coefficients come from the library's host function, brov_rotor_coeffs).
Prints the RMS position error of the shipped controller against rotors with tau = 0.2 s (the reference's), 0.1 s and 0.05 s and against
tau = 0 (every command becomes force at once: the loop without the stage), over 40 / 80 / 120 ticks, and the RMS gap between the commanded
and the applied thrusts (in the units of the result record's thrust field)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import trajectory_oracle as T                      # noqa: E402
from oracle.oracle_ffi import Oracle, build                     # noqa: E402
from delay_restatement import rms_position_error                # noqa: E402
from rotor_restatement import RotorRestatement, cpu_rotor_loop  # noqa: E402
import bluerov2_amd                                             # noqa: E402
from bluerov2_amd.solver import P_NOMINAL                       # noqa: E402


def main():
    build()
    bluerov2_amd.build_library()
    orc = Oracle()
    N, B, h = 20, 4, 0.05
    rng = np.random.default_rng(21)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
    pp = np.tile(P_NOMINAL, (B, 1))

    def run(tau, ticks):
        """(RMS position error, worst status, RMS of commanded - applied thrust, first tick after which a state is not finite or None)"""
        a, b = bluerov2_amd.rotor_coeffs(tau, h)
        ro = RotorRestatement(B, a, b)
        with np.errstate(all="ignore"):
            log = cpu_rotor_loop(orc, ro, traj, x0, P_NOMINAL, pp, N, ticks, dt=h)
        bad = np.nonzero(~np.isfinite(log["x"]).all(axis=(1, 2)))[0]
        return (rms_position_error(log["x"], traj), int(np.abs(log["status"]).max()), float(np.sqrt(ro.lag_sq.sum() / (ticks * B * 6))),
                (int(bad[0]) - 1 if len(bad) else None))

    print("ticks   tau = 0    tau = 0.05 s   tau = 0.1 s   tau = 0.2 s   (RMS position error; in brackets the RMS gap |c - m| in the record's thrust units)")
    for ticks in (40, 80, 120):
        cells = [run(tau, ticks) for tau in (0.0, 0.05, 0.1, 0.2)]
        print(f"{ticks:5d}   " + "   ".join(
            (f"{c[0]:.4f} m [{c[2]:.3f}]" if c[3] is None else f"not finite behind tick {c[3]}") + ("" if c[1] == 0 else f" (status {c[1]})")
            for c in cells))


if __name__ == "__main__":
    main()
