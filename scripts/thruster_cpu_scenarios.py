#!/usr/bin/env python3
"""The thruster scenarios of DESIGN.md section 4.9b on the CPU loop (tests/thruster_restatement.py: oracle RTI step, restated stage and plant,
oracle EKF configured as tests/test_gpu_plant_wrench.py::_ekf_pair): N = 20, B = 4, seed 21, circle, 80 ticks.  Needs no GPU.
Prints the RMS position error of every scenario with and without the hand-off of the estimate, and the clip count of the +-100 run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import trajectory_oracle as T                      # noqa: E402
from oracle.oracle_ffi import EkfOracle, Oracle, build          # noqa: E402
from thruster_restatement import ThrusterRestatement, cpu_thruster_loop   # noqa: E402
from bluerov2_amd.solver import P_NOMINAL                                 # noqa: E402


def ekf():
    e = EkfOracle(); e.par.compensate_coef = 1.0; e.par.rotor_constant = 1.0
    for j in range(12, 24):
        e.par.K[j] = 0.0
    return e


def main():
    build()
    orc = Oracle()
    N, B, ticks = 20, 4, 80
    rng = np.random.default_rng(21)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
    pp = np.tile(P_NOMINAL, (B, 1))

    def rms(thr, handoff, n=ticks):
        log = cpu_thruster_loop(orc, ekf(), thr, traj, x0, P_NOMINAL, pp, N, n, handoff=handoff)
        assert not log["status"].any()
        err = log["x"][1:, :, :3] - traj[1:n + 1, None, :3]
        return float(np.sqrt((err ** 2).sum(-1).mean()))

    dead, weak = np.ones(6), np.ones(6)
    dead[0], weak[0] = 0.0, 0.5
    for name, kw in (("healthy", {}), ("thruster 0 dead from tick 10", dict(gain=dead, onset=10)), ("thruster 0 at half gain from tick 10", dict(gain=weak, onset=10))):
        print(f"{name:40s} RMS position error {rms(ThrusterRestatement(B, **kw), True):.4f} m with the hand-off, "
              f"{rms(ThrusterRestatement(B, **kw), False):.4f} m without")
    thr = ThrusterRestatement(B, lo=-100.0, hi=100.0)
    rms(thr, True, 30)
    print(f"limits +-100, 30 ticks, hand-off on: {thr.clip_ticks.sum()} of {6 * B * 30} commands clip")


if __name__ == "__main__":
    main()
