#!/usr/bin/env python3
"""The thrust-curve scenarios of DESIGN.md section 4.9j on the CPU loop (tests/curve_restatement.py: the oracle's RTI step, the restated curve
stage, the oracle's model as plant, the oracle EKF configured as scripts/thruster_cpu_scenarios.py has it): N = 20, B = 4, seed 21, the
circle, Ts = 0.05, the setup of scripts/rotor_cpu_scenarios.py.  Needs no GPU.
The shipped controller flies 40 and 120 ticks on
  (a) the linear plant (the stage a copy);
  (b) BASIC, k = 1 / C_NOM: the quadratic meets the linear curve at the nominal command C_NOM = 30 (in the record's thrust units);
  (c) the T200 table (tests/golden/t200_16v.json) behind a linear PWM map -- full forward thrust at +400 us -- in 4 us steps, no pre-map;
  (d) the same with inverse_table() of the table as the pre-map;
  (e) the reference's own numbers: its simulated thruster gives rotorConstant w |w| = 1e-4 w |w| N for the command w the node publishes,
      the model assumes rc w N (rc = the model's rotor constant): BASIC with k = 1e-4 / rc
with and without the EKF hand-off, and prints the RMS position error, the dead ticks and the charge.  Units: one thrust unit of the record is
rc N, so 1 kgf is 9.80665 / rc of them: the table's efficiency.
Then the impulse error of evaluating the curve at the rotor stage's MEAN command of a step: plant (b) behind rotors of tau = 0.2 s; per step
and thruster k m |m| against the mean of k r(s) |r(s)| over the step, r(s) = c + (r0 - c) exp(-s / tau) at 1000 midpoints; the worst over the run."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import trajectory_oracle as T                      # noqa: E402
from oracle.oracle_ffi import EkfOracle, Oracle, build          # noqa: E402
from delay_restatement import rms_position_error                # noqa: E402
from curve_restatement import BASIC, PRE_POLY, PRE_TABLE, TABLE, CurveRestatement, cpu_curve_loop, table_slopes   # noqa: E402
from rotor_restatement import RotorRestatement                  # noqa: E402
import bluerov2_amd                                             # noqa: E402
from bluerov2_amd.solver import P_NOMINAL, ROTOR_CONSTANT       # noqa: E402

C_NOM = 30.0
KGF = 9.80665 / ROTOR_CONSTANT            # thrust units per kgf
PWM_PER_UNIT = 400.0 / (5.25 * KGF)       # the linear map: full forward thrust at +400 us


def ekf():
    e = EkfOracle(); e.par.compensate_coef = 1.0; e.par.rotor_constant = 1.0
    for j in range(12, 24):
        e.par.K[j] = 0.0
    return e


def main():
    build()
    bluerov2_amd.build_library()
    orc = Oracle()
    N, B, h = 20, 4, 0.05
    rng = np.random.default_rng(21)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
    pp = np.tile(P_NOMINAL, (B, 1))
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "t200_16v.json")))
    x, y, a = bluerov2_amd.curve_from_pwm_table(d["pwm"], d["kgf"], d["amps"])
    cur = dict(x=x, y=y, slope=table_slopes(x, y), amps=a, amps_slope=table_slopes(x, a))
    ix, iy = bluerov2_amd.inverse_table(x, y * KGF)
    pre = dict(x=ix, y=iy, slope=table_slopes(ix, iy))
    plants = (("(a) linear", lambda: CurveRestatement(B)),
              ("(b) BASIC, k = 1 / 30", lambda: CurveRestatement(B, kind=BASIC, k=1.0 / C_NOM)),
              ("(c) T200, linear PWM map, 4 us", lambda: CurveRestatement(B, kind=TABLE, pre=PRE_POLY, pre_poly=(0.0, 0.0, 0.0, PWM_PER_UNIT, 0.0),
                                                                           quantum=4.0, eff=KGF, curve=cur)),
              ("(d) T200, inverse pre-map, 4 us", lambda: CurveRestatement(B, kind=TABLE, pre=PRE_TABLE, quantum=4.0, eff=KGF, curve=cur, pre_table=pre)),
              ("(e) BASIC, k = 1e-4 / rc", lambda: CurveRestatement(B, kind=BASIC, k=1e-4 / ROTOR_CONSTANT)))
    print(f"thrust units per kgf {KGF:.3f}; linear PWM map {PWM_PER_UNIT:.5f} us per unit; the curves of (e) meet at a command of {ROTOR_CONSTANT / 1e-4:.2f} units")
    print("plant                              hand-off   RMS 40 ticks   RMS 120 ticks   dead ticks (of %d)   charge [A s], mean   worst status" % (120 * B * 6))
    for name, make in plants:
        for handoff in (False, True):
            cv = make()
            with np.errstate(all="ignore"):
                log = cpu_curve_loop(orc, cv, traj, x0, P_NOMINAL, pp, N, 120, dt=h, ekf=ekf(), handoff=handoff)
            bad = np.nonzero(~np.isfinite(log["x"]).all(axis=(1, 2)))[0]
            r40 = "not finite" if len(bad) and bad[0] <= 40 else f"{rms_position_error(log['x'][:41], traj):.4f} m"
            r120 = f"not finite behind tick {bad[0] - 1}" if len(bad) else f"{rms_position_error(log['x'], traj):.4f} m"
            if name.startswith("(a)") and not handoff:
                t = np.abs(log["applied_t"])                 # the stage is a copy: the commanded thrusts
                first = f"commands on the linear plant, no hand-off: median |t| {np.median(t):.2f} units, 90th percentile {np.percentile(t, 90):.2f}, largest {t.max():.2f}"
            print(f"{name:34s} {'on ' if handoff else 'off'}        {r40:12s}   {r120:13s}   {int(cv.dead_ticks.sum()):6d}               "
                  f"{cv.charge.mean():8.3f}             {int(np.abs(log['status']).max())}"
                  + ("" if log["ekf_failed"] < 0 else f"   (the observer gave up at tick {log['ekf_failed']})"))
    print(first)
    # ---- the impulse error of the curve at the mean command ---------------------------------------------------------------------------
    tau = 0.2
    al, be = bluerov2_amd.rotor_coeffs(tau, h)
    cv, ro = CurveRestatement(B, kind=BASIC, k=1.0 / C_NOM), RotorRestatement(B, al, be)
    log = cpu_curve_loop(orc, cv, traj, x0, P_NOMINAL, pp, N, 120, dt=h, ro=ro)
    r0, c = log["rotor_from"], log["rotor_cmd"]
    s = (np.arange(1000) + 0.5) * (h / 1000.0)
    r = c[..., None] + (r0 - c)[..., None] * np.exp(-s / tau)
    exact = (r * np.abs(r)).mean(axis=-1) / C_NOM
    m = c + be * (r0 - c)
    at_mean = m * np.abs(m) / C_NOM
    err = np.abs(at_mean - exact)
    j = np.unravel_index(np.argmax(err), err.shape)
    print(f"impulse error of BASIC at the rotors' mean command (tau = {tau} s, k = 1 / {C_NOM:g}, 120 ticks): worst |k m|m| - mean k r|r|| = "
          f"{err.max():.4f} thrust units at tick {j[0]} (the exact mean there {exact[j]:.3f}, the command {c[j]:.3f}, from {r0[j]:.3f}); "
          f"RMS {np.sqrt((err ** 2).mean()):.5f}; RMS of the exact mean {np.sqrt((exact ** 2).mean()):.3f}")


if __name__ == "__main__":
    main()
