#!/usr/bin/env python3
"""The input-delay scenarios of DESIGN.md section 4.9e on the CPU loop (tests/delay_restatement.py: the oracle's RK4 as predictor, the
oracle's RTI step, the restated queue, the oracle's model as plant): N = 20, B = 4, seed 21, the circle, Ts = 0.05.  Needs no GPU.
Prints the RMS position error of the undelayed loop, of a 2-tick input delay without prediction and of the same delay predicted through,
over 40 / 60 / 80 ticks, and the 120-tick runs of the mismatched cases (delay 1; delay 1 predicted 3; delay 3 predicted 1)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import trajectory_oracle as T                      # noqa: E402
from oracle.oracle_ffi import Oracle, build                     # noqa: E402
from delay_restatement import DelayRestatement, cpu_delay_loop, rms_position_error   # noqa: E402
from bluerov2_amd.solver import P_NOMINAL                       # noqa: E402


def main():
    build()
    orc = Oracle()
    N, B = 20, 4
    rng = np.random.default_rng(21)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
    pp = np.tile(P_NOMINAL, (B, 1))

    def run(delay, comp, ticks):
        """(RMS position error, worst status, first tick after which a state is not finite or None)"""
        with np.errstate(all="ignore"):
            log = cpu_delay_loop(orc, DelayRestatement(B, delay, comp), traj, x0, P_NOMINAL, pp, N, ticks)
        bad = np.nonzero(~np.isfinite(log["x"]).all(axis=(1, 2)))[0]   # (row j of the state log: the state after tick j - 1)
        return rms_position_error(log["x"], traj), int(np.abs(log["status"]).max()), (int(bad[0]) - 1 if len(bad) else None)

    print("ticks   no delay   2-tick delay, no prediction   2-tick delay, predicted 2 ticks")
    for ticks in (40, 60, 80):
        cells = [run(0, 0, ticks), run(2, 0, ticks), run(2, 2, ticks)]
        assert not any(c[1] for c in cells)
        print(f"{ticks:5d}   {cells[0][0]:.4f} m   {cells[1][0]:.4f} m                    {cells[2][0]:.4f} m")
    print("120 ticks:")
    for name, delay, comp in (("no delay", 0, 0), ("delay 1, no prediction", 1, 0), ("delay 2, no prediction", 2, 0), ("delay 2, predicted 2", 2, 2),
                              ("delay 1, predicted 3 (over-prediction)", 1, 3), ("delay 3, predicted 1 (under-prediction)", 3, 1)):
        rms, status, bad = run(delay, comp, 120)
        tail = f"not finite behind tick {bad}" if bad is not None else f"RMS position error {rms:.4f} m"
        print(f"  {name:42s} {tail}, worst status {status}")


if __name__ == "__main__":
    main()
