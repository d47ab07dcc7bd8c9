#!/usr/bin/env python3
"""The Coriolis scenario of DESIGN.md section 4.9g on the CPU loop (tests/coriolis_restatement.py: the oracle's RTI step, the oracle's model
under the restated force as plant, the oracle EKF configured as tests/test_gpu_plant_wrench.py::_ekf_pair): N = 20, B = 4, seed 21, the circle
from a level start, 80 ticks, no external disturbance, the observer's estimate handed to the controller.  Needs no GPU.
Prints, for the stage off, RIGID and RIGID|ADDED, the median |estimate| of the observer over the last 20 ticks per channel: what the observer
reports although nothing pushes the vehicle."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle.oracle_ffi import Oracle, build                     # noqa: E402
import coriolis_restatement as CO                               # noqa: E402

P_NOMINAL = np.array([0, 0, 0, 0, 1.7182, 0, 5.468, 0.4006, -11.7391, -20, -31.8678, -5, -18.18, -21.66, -36.99, -1.55])


def main():
    build()
    orc = Oracle()
    N, B, ticks = 20, 4, 80
    traj, x0 = CO.scenario_inputs(B)
    pp = np.tile(P_NOMINAL, (B, 1))
    print("plant                 median |estimate| over the last 20 ticks:   X [N]      Y [N]      Z [N]    N [N m]   worst status")
    for name, terms in (("stage off", 0), ("RIGID", CO.RIGID), ("RIGID|ADDED", CO.RIGID | CO.ADDED)):
        log = CO.cpu_dob_loop(orc, CO.ekf_for_the_device_plant(), terms, traj, x0, P_NOMINAL, pp, N, ticks)
        m = CO.phantom_medians(log["est"])
        print(f"{name:20s}                                          {m[0]:9.4f}  {m[1]:9.4f}  {m[2]:9.4f}  {m[5]:9.4f}   {int(np.abs(log['status']).max())}")


if __name__ == "__main__":
    main()
