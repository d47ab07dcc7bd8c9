#!/usr/bin/env python3
"""The error-state filter at its sensors' own rates against the single-rate hand-off, as the observer of a DOB loop on the circle under the
constant world-frame force of DESIGN.md section 4.4b's table (scripts/eskf_cpu_scenarios.py, whose loop and report this script reuses).

CPU part (no GPU): the oracle's RTI step as controller, the oracle's RK4 of the OCP model as plant, the numpy filter (tests/eskf_exact.py).
  single rate: one plant step and one update tick per control tick, the filter's dt = gps_dt = 0.05 (that script's loop);
  sensors' rates: imu_per_tick = 5 plant steps of h = 0.01 per control tick, the IMU/GPS stage's numpy restatement (tests/imu_restatement.py)
  behind each, gps_every = 3; a predict-only tick where the stage has no fix, an update tick where it has one; the filter's dt = h;
  without noise, and with noise, bias and dropped fixes (dropout 0.2).
Reported as there: the world-frame estimate averaged over the last 50 control ticks, its error against the applied force, the RMS position
error.  The reference's injection (vel_inject = 2, biases and gravity not injected), P symmetrised after every tick as the device returns it.

--device: the same two loops on the device at B = 4: brov_eskf_update_from_solver per control tick, and brov_closed_loop_eskf."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import eskf_exact as X                                          # noqa: E402
import eskf_cpu_scenarios as S                                  # noqa: E402
from imu_restatement import ImuRestatement                      # noqa: E402

PER_TICK, EVERY = 5, 3
H = S.TS / PER_TICK
SIGMA = np.array([0.02] * 3 + [0.002] * 3 + [0.05] * 3 + [0.01] * 3)
BIAS = np.array([0.01, -0.02, 0.015, 1e-3, -2e-3, 5e-4])
DROPOUT = 0.2


def rates_params():
    v = S.loop_params(2.0, 0.0)
    v[0] = H                       # dt: the IMU period; gps_dt is not read at the sensors' rates (the stage differences the fixes)
    return v


def cpu_rates_loop(orc, traj, noisy):
    op = orc.opts(S.N, S.TS)
    x, u, pi, lam = orc.init_iterate(op)
    xs = np.zeros(12); xs[:6] = traj[0, :6]
    p = np.tile(S.P_NOMINAL, (S.N + 1, 1))
    par = X.par_dict(rates_params())
    r = ImuRestatement(1, H, gps_every=EVERY, seed=1, sigma=SIGMA if noisy else None, bias=BIAS if noisy else None,
                       dropout=DROPOUT if noisy else None)
    r.restart(0, xs[None])
    fx = np.zeros(X.NX); fx[6] = 1.0; fx[18] = -par["g"]
    fP = np.zeros((X.NE, X.NE))
    est, xlog, m = np.zeros((S.TICKS, 3)), np.zeros((S.TICKS, 12)), 0
    for k in range(S.TICKS):
        u0 = orc.rti_step(op, xs, traj[k:k + S.N + 1], p, x, u, pi, lam)["u0"]
        for _ in range(PER_TICK):
            pl = S.P_NOMINAL.copy()
            pl[0:3] = X.np_rot_euler(*xs[3:6]).T @ S.FORCE
            xs = orc.rk4(xs, u0, pl, H)
            m += 1
            fix = r.refresh(m, xs[None])[0]
            d = X.np_tick(par, fx, fP, r.imu[0], r.gps_p[0], r.gps_v[0], r.q_meas[0], X.np_thrust(u0), update=bool(fix))
            fx, fP = d["x_new"], X.from_triu(X.to_triu(d["P_new"]))
        est[k], xlog[k] = d["xi_world"], xs
        p[:, 0:4] = d["mpc_p"]
    print(f"    ({int(r.fixes[0])} fixes taken, {int(r.dropped[0])} dropped of {int(r.samples[0])} samples)")
    return est, xlog


def device_rates_loop(ba, traj, noisy):
    B = 4
    s = ba.BatchSolver(B, ba.SolverOptions(S.N, S.TS), device=0)
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_trajectory(traj)
    s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1)))      # the plant keeps its own parameters: it must not read the estimate back
    s.set_plant_wrench(constant=np.concatenate([S.FORCE, np.zeros(3)]))
    s.set_imu(H, gps_every=EVERY, seed=1, sigma=SIGMA if noisy else None, bias=BIAS if noisy else None, dropout=DROPOUT if noisy else None)
    e = ba.BatchEskf(B, X.par_apply(ba.EskfParams.default(), rates_params()))
    out = ba.closed_loop_eskf(s, e, S.TICKS, line0=0, ncols=16, dt=S.TS, imu_per_tick=PER_TICK)
    st = s.imu_stats()
    print(f"    (instance 0: {int(st['fixes'][0])} fixes taken, {int(st['dropped'][0])} dropped of {int(st['samples'][0])} samples)")
    e.close(); s.close()
    return out["est"][:, 0], out["x"][1:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    a = ap.parse_args()
    from oracle import trajectory_oracle as T
    traj = T.circle()
    print(f"constant world-frame force {tuple(float(v) for v in S.FORCE)} N on the circle, {S.TICKS} control ticks, figures over the last {S.TAIL}; "
          f"sensors' rates: imu_per_tick = {PER_TICK}, gps_every = {EVERY}")
    if not a.device:
        from oracle.oracle_ffi import Oracle, build
        build()
        orc = Oracle()
        print("CPU loop (oracle RTI step, oracle RK4 plant, numpy filter, P symmetrised every tick):")
        S.report("single rate: one update tick per control tick", *S.cpu_loop(orc, traj, ("eskf", S.loop_params(2.0, 0.0), True)), traj)
        S.report("sensors' rates, no noise", *cpu_rates_loop(orc, traj, False), traj)
        S.report("sensors' rates, noise, bias, dropout 0.2", *cpu_rates_loop(orc, traj, True), traj)
    else:
        import bluerov2_amd as ba
        print("device loop, B = 4:")
        S.report("single rate: brov_eskf_update_from_solver per tick", *S.device_loop(ba, traj, "eskf", S.loop_params(2.0, 0.0)), traj)
        S.report("sensors' rates (brov_closed_loop_eskf), no noise", *device_rates_loop(ba, traj, False), traj)
        S.report("sensors' rates, noise, bias, dropout 0.2", *device_rates_loop(ba, traj, True), traj)


if __name__ == "__main__":
    main()
