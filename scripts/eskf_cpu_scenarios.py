#!/usr/bin/env python3
"""The error-state filter as the observer of a DOB loop on the circle under a constant world-frame force.

CPU part (no GPU): the oracle's RTI step as controller, the oracle's RK4 of the OCP model as plant -- the force enters as the model's own
disturbance, turned into the body frame at the start of every plant step --, the numpy restatement of the filter (tests/eskf_exact.py) fed by
its restated hand-off, its estimate handed to the controller's p[0..2] (compensate_coef = rotor_constant = 1, dt = gps_dt = 0.05).  N = 20,
Ts = 0.05, one vehicle, 200 ticks.  Reported: the world-frame estimate R(q) xi averaged over the last 50 ticks against the applied force, and
the RMS position error over them, with the reference's injection (vel_inject = 2, biases and gravity not injected) and with the textbook one
(vel_inject = 1, inject_bias_g = 1), each with the covariance as the reference's (I - K H) P leaves it in double -- not symmetric to the last
bit, and over 200 ticks that shows -- and with it symmetrised after every tick, which is what the device returns; beside them the 18-state EKF (the C oracle's filter, its own hand-off) observing the same kind of run,
and the loop without an observer.

--device: the same loop composed on the device from brov_solve, brov_plant_step under brov_plant_wrench_*, brov_eskf_update_from_solver and
brov_eskf_apply_to_solver at B = 4, and the 18-state observer through brov_ekf_*; the figures stand beside the CPU ones."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import eskf_exact as X                                          # noqa: E402

N, TS, TICKS, TAIL = 20, 0.05, 200, 50
FORCE = np.array([4.0, -3.0, 2.0])
P_NOMINAL = np.array([0, 0, 0, 0, 1.7182, 0, 5.468, 0.4006, -11.7391, -20, -31.8678, -5, -18.18, -21.66, -36.99, -1.55])


def loop_params(vel_inject, inject_bias_g):
    v = X.default_par_vector()
    d = {f: sum(n for _, n in X.PAR_FIELDS[:k]) for k, (f, n) in enumerate(X.PAR_FIELDS)}
    for f, val in (("dt", TS), ("gps_dt", TS), ("compensate_coef", 1.0), ("rotor_constant", 1.0), ("vel_inject", vel_inject),
                   ("inject_bias_g", inject_bias_g)):
        v[d[f]] = val
    return v


def report(name, est_world, xlog, traj):
    est = est_world[-TAIL:].mean(axis=0)
    rms = np.sqrt(((xlog[-TAIL:, :3] - traj[TICKS - TAIL + 1:TICKS + 1, :3]) ** 2).sum(axis=1).mean())
    print(f"  {name:58s} estimate ({est[0]:+7.3f}, {est[1]:+7.3f}, {est[2]:+7.3f}) N  error {np.linalg.norm(est - FORCE):6.3f} N  "
          f"RMS position error {rms:.4f} m")


def cpu_loop(orc, traj, observer):
    """observer: None, ("eskf", par_vec, P symmetrised after every tick?) or ("ekf", oracle filter).  Returns (world-frame estimates [ticks, 3], states [ticks, 12])"""
    op = orc.opts(N, TS)
    x, u, pi, lam = orc.init_iterate(op)
    xs = np.zeros(12); xs[:6] = traj[0, :6]
    p = np.tile(P_NOMINAL, (N + 1, 1))
    est, xlog, failed = np.zeros((TICKS, 3)), np.zeros((TICKS, 12)), None
    if observer and observer[0] == "eskf":
        par = X.par_dict(observer[1])
        fx = np.zeros(X.NX); fx[6] = 1.0; fx[18] = -par["g"]
        fP, vprev, pprev = np.zeros((X.NE, X.NE)), None, None
    if observer and observer[0] == "ekf":
        ex, eP = observer[1].init_state(1)
        ex[0, :12], ex[0, 12:] = xs, 0.0      # started at the plant's state with no disturbance, like the error-state filter beside it
        vb_prev = np.zeros(6)
    for k in range(TICKS):
        r = orc.rti_step(op, xs, traj[k:k + N + 1], p, x, u, pi, lam)
        u0 = r["u0"]
        pl = P_NOMINAL.copy()
        pl[0:3] = X.np_rot_euler(*xs[3:6]).T @ FORCE
        xs = orc.rk4(xs, u0, pl, TS)
        if observer and observer[0] == "eskf":
            imu, gp, gv, qm, th, vI = X.np_inputs_from_state(par, xs, X.np_thrust(u0), vprev, pprev)
            d = X.np_tick(par, fx, fP, imu, gp, gv, qm, th)
            fx, fP, vprev, pprev = d["x_new"], d["P_new"], vI, gp
            if observer[2]:      # as the device returns it: the upper triangle mirrored over the lower one
                fP = X.from_triu(X.to_triu(fP))
            est[k] = d["xi_world"]
            p[:, 0:4] = d["mpc_p"]
        elif observer:
            acc = (xs[6:12] - vb_prev) / TS
            vb_prev = xs[6:12].copy()
            wf, mp, rc = observer[1].update(ex, eP, X.np_thrust(u0)[None], xs[None], acc[None])
            if rc != 0:      # the oracle's filter gives up (its covariance has left the doubles): said, and the loop goes on with the last hand-off
                if failed is None:
                    failed = k
                    print(f"  (the 18-state filter fails from tick {k} on: max |P| = {np.abs(eP).max():.1e}; the estimate below is its last one)")
                est[k], xlog[k] = est[k - 1], xs
                continue
            est[k] = wf[0, :3]
            p[:, 0:4] = mp[0]
        xlog[k] = xs
    return est, xlog


def device_loop(ba, traj, kind, par_vec=None):
    B = 4
    s = ba.BatchSolver(B, ba.SolverOptions(N, TS), device=0)
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    s.set_x0(x0); s.set_params(ba.P_NOMINAL)
    s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1)))      # the plant keeps its own parameters: it must not read the estimate back
    s.set_plant_wrench(constant=np.concatenate([FORCE, np.zeros(3)]))
    obs = None
    if kind == "eskf":
        obs = ba.BatchEskf(B, X.par_apply(ba.EskfParams.default(), par_vec))
    elif kind == "ekf":
        q = ba.EkfParams.default(); q.compensate_coef = 1.0; q.rotor_constant = 1.0
        for j in range(18, 30):
            q.K[j] = 0.0           # as in the CPU loop
        obs = ba.BatchEkf(B, q)
        xe = np.zeros(18); xe[:6] = traj[0, :6]
        obs.reset(xe, np.eye(18))
    est, xlog = np.zeros((TICKS, 3)), np.zeros((TICKS, 12))
    for k in range(TICKS):
        s.set_yref(traj[k:k + N + 1])
        s.solve()
        s.plant_step(TS)
        if obs is not None:
            obs.update_from_solver(s)
            obs.apply_to_solver(s)
            est[k] = obs.outputs()[1][0] if kind == "eskf" else obs.outputs()[0][0, :3]
        xlog[k] = s.get_x0()[0]
    return est, xlog


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    a = ap.parse_args()
    from oracle import trajectory_oracle as T
    traj = T.circle()
    print(f"constant world-frame force {tuple(float(v) for v in FORCE)} N on the circle, {TICKS} ticks, figures over the last {TAIL}")
    if not a.device:
        from oracle.oracle_ffi import EkfOracle, Oracle, build
        build()
        orc = Oracle()
        print("CPU loop (oracle RTI step, oracle RK4 plant, numpy filter):")
        report("no observer", *cpu_loop(orc, traj, None), traj)
        for sym, tag in ((False, "P as (I - K H) P leaves it"), (True, "P symmetrised every tick")):
            report(f"ESKF, reference's injection, {tag}", *cpu_loop(orc, traj, ("eskf", loop_params(2.0, 0.0), sym)), traj)
            report(f"ESKF, textbook injection, {tag}", *cpu_loop(orc, traj, ("eskf", loop_params(1.0, 1.0), sym)), traj)
        eo = EkfOracle()
        eo.par.compensate_coef = 1.0; eo.par.rotor_constant = 1.0
        for j in range(18, 30):
            eo.par.K[j] = 0.0      # rows 3, 4 of K zeroed: with the OCP model as plant the filter diverges otherwise
        eo.lib.orc_ekf_derive(eo.par)
        report("18-state EKF (C oracle)", *cpu_loop(orc, traj, ("ekf", eo)), traj)
    else:
        import bluerov2_amd as ba
        print("device loop, B = 4 (brov_solve, brov_plant_step under the wrench, brov_eskf_update_from_solver, brov_eskf_apply_to_solver):")
        report("no observer", *device_loop(ba, traj, None), traj)
        report("ESKF, the reference's injection (vel_inject 2, no bias inj.)", *device_loop(ba, traj, "eskf", loop_params(2.0, 0.0)), traj)
        report("ESKF, the textbook injection (vel_inject 1, bias inj.)", *device_loop(ba, traj, "eskf", loop_params(1.0, 1.0)), traj)
        report("18-state EKF (brov_ekf_*)", *device_loop(ba, traj, "ekf"), traj)


if __name__ == "__main__":
    main()
