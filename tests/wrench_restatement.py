"""CPU restatement of the plant's time-varying world-frame wrench (include/bluerov2_nmpc.h, brov_plant_wrench_*; the scenarios of the
reference's applyBodyWrench(), bluerov2_dobmpc/src/bluerov2_dob.cpp:754-892), the yardstick of bluerov2_amd/csrc/plant_wrench.hip.

Generator: a pure function of (mode data, instance b, tick k), every operation one IEEE FP64 operation in the order the header states
it (numpy elementwise arithmetic never contracts into FMAs); the 64-bit mixing in np.uint64, which wraps around.  sin() is libm's
(math.sin): the one step in which the device may differ, by about an ulp.

Plant: ERK4 over one control period that calls the oracle's f6(x, u, p, drp) once per stage, with p[0..3] and drp augmented by the
world wrench projected into the body frame with THAT stage's attitude, f_b = R^T f_w, t_b = R^T t_w (R as bluerov2.py:103-111 writes
it: the matrix of the kinematic rows).
"""
import math

import numpy as np

OFF, CONSTANT, PERIODIC, TABLE = 0, 1, 2, 3
GOLDEN_GAMMA = np.uint64(0x9E3779B97F4A7C15)


def splitmix64_finalise(z):
    """output function of SplitMix64 on an array of np.uint64 (wrap-around arithmetic)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


class WrenchRestatement:
    def __init__(self, B):
        self.B = int(B)
        self.mode = OFF

    def constant(self, w):
        w = np.asarray(w, dtype=np.float64)
        self.w = np.ascontiguousarray(np.broadcast_to(w, (self.B, 6)))
        self.mode = CONSTANT
        return self

    def periodic(self, seed=0, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0):
        self.seed, self.scale, self.phase0, self.dphi, self.tz_div = np.uint64(seed), float(scale), float(phase0), float(dphi), float(tz_div)
        self.mode = PERIODIC
        return self

    def table(self, tab, gain=None):
        self.tab = np.ascontiguousarray(tab, dtype=np.float64)
        assert self.tab.ndim == 2 and self.tab.shape[1] == 6
        self.gain = None if gain is None else np.asarray(gain, dtype=np.float64).reshape(self.B)
        self.mode = TABLE
        return self

    # ---- periodic mode, piece by piece ------------------------------------------------------------------------------------
    def phase(self, k):
        """t_k = phase0 + k * dphi: a product, not the reference's running sum"""
        return self.phase0 + float(k) * self.dphi

    def half_period(self, k):
        j = int(math.floor(self.phase(k) / math.pi))
        assert 0 <= j < 2 ** 22
        return j

    def amplitudes(self, k):
        """[B][4]: A_X, A_Y, A_Z, A_N of every instance in the half period tick k lies in"""
        j = self.half_period(k)
        b = np.arange(self.B, dtype=np.uint64)[:, None]
        c = np.arange(4, dtype=np.uint64)[None, :]
        n = (b << np.uint64(24)) | (np.uint64(j) << np.uint64(2)) | c
        with np.errstate(over="ignore"):
            z = splitmix64_finalise(self.seed + (n + np.uint64(1)) * GOLDEN_GAMMA)
        U = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        return self.scale * (0.5 + 0.5 * U)

    def sin_phase(self, k):
        return math.sin(self.phase(k))

    # ---- the wrench -----------------------------------------------------------------------------------------------------------
    def wrench(self, k):
        """[B][6] world-frame [fx fy fz tx ty tz] at tick k"""
        if self.mode == OFF:
            return np.zeros((self.B, 6))
        if self.mode == CONSTANT:
            return self.w.copy()
        if self.mode == TABLE:
            row = self.tab[min(max(int(k), 0), self.tab.shape[0] - 1)]
            g = np.ones(self.B) if self.gain is None else self.gain
            return row[None, :] * g[:, None]
        A = self.amplitudes(k)
        sn = self.sin_phase(k)
        w = np.zeros((self.B, 6))
        w[:, 0], w[:, 1], w[:, 2] = sn * A[:, 0], sn * A[:, 1], sn * A[:, 2]
        w[:, 5] = w[:, 1] / self.tz_div          # the yaw torque follows the Y amplitude (bluerov2_dob.cpp:787); A_N is drawn, never used
        return w


def rotation(x):
    """body -> world rotation of the model's kinematic rows (bluerov2.py:103-111), from x[3:6] = roll, pitch, yaw"""
    sph, cph, sth, cth, sps, cps = math.sin(x[3]), math.cos(x[3]), math.sin(x[4]), math.cos(x[4]), math.sin(x[5]), math.cos(x[5])
    return np.array([[cps * cth, -sps * cph + cps * sth * sph, sps * sph + cps * cph * sth],
                     [sps * cth, cps * cph + sph * sth * sps, -cps * sph + sth * sps * cph],
                     [-sth, cth * sph, cth * cph]])


def f_under_wrench(oracle, x, u, p, w, drp=None):
    """the oracle's model with the world wrench w[6] projected with the attitude of x"""
    R = rotation(x)
    fb, tb = R.T @ w[:3], R.T @ w[3:]
    pa = np.array(p, dtype=np.float64, copy=True)
    pa[0] += fb[0]; pa[1] += fb[1]; pa[2] += fb[2]; pa[3] += tb[2]
    d = np.zeros(2) if drp is None else np.asarray(drp, dtype=np.float64)
    return oracle.f6(x, u, pa, np.array([d[0] + tb[0], d[1] + tb[1]]))


def rk4_under_wrench(oracle, x, u, p, w, dt, substeps=1, drp=None):
    """one control period of the plant: `substeps` ERK4 steps, the wrench held, projected afresh at every stage"""
    x = np.array(x, dtype=np.float64, copy=True)
    h = dt / substeps
    for _ in range(substeps):
        k1 = f_under_wrench(oracle, x, u, p, w, drp)
        k2 = f_under_wrench(oracle, x + 0.5 * h * k1, u, p, w, drp)
        k3 = f_under_wrench(oracle, x + 0.5 * h * k2, u, p, w, drp)
        k4 = f_under_wrench(oracle, x + h * k3, u, p, w, drp)
        x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return x


def plant_step(oracle, x, u, p, w, dt, substeps=1):
    """batched: x [B][12], u [B][4], p [B][16], w [B][6]"""
    return np.stack([rk4_under_wrench(oracle, x[b], u[b], p[b], w[b], dt, substeps) for b in range(len(x))])


def cpu_dob_loop(oracle, ekf, wrench, traj, x0, p_ctrl, p_true, N, ticks, line0=0, dt=0.05, substeps=1, handoff=True, Ts=None):
    """The DOB control loop on the CPU, tick for tick what brov_closed_loop_dob enqueues with r == NULL: window(line0 + k) -> the
    oracle's RTI step -> the restated plant under wrench.wrench(k) -> the oracle EKF fed with the new plant state, the thrust allocation
    of the applied input and (v - v_prev) / dt (v_prev = 0 at the start) -> p[0..3] of every stage := the EKF's hand-off (skipped with
    handoff=False: the uncompensated controller).  `ekf` is an EkfOracle configured like the device observer.  Returns
    dict(u [ticks][B][4], x [ticks+1][B][12], status [ticks][B], wrench [ticks][B][6], est [ticks][B][6], mpc_p [ticks][B][4])."""
    from oracle import trajectory_oracle as T
    B = len(x0)
    op = oracle.opts(N, Ts)
    x, u, pi, lam = oracle.init_iterate(op, B)
    pfull = np.ascontiguousarray(np.broadcast_to(np.asarray(p_ctrl, dtype=np.float64).reshape(-1, 16)[:, None, :], (B, N + 1, 16)))
    xe, Pe = ekf.init_state(B)
    xc = np.array(x0, dtype=np.float64, copy=True)
    vprev = np.zeros((B, 6))
    rotor = 0.026546960744430276
    log = dict(u=[], x=[xc.copy()], status=[], wrench=[], est=[], mpc_p=[])
    res = None
    for k in range(ticks):
        yref = np.ascontiguousarray(np.broadcast_to(T.window(traj, line0 + k, N), (B, N + 1, 16)))
        _, res = oracle.rti_step_batch(op, xc, yref, pfull, x, u, pi, lam, res_prev=res)
        u0 = res["u0"].copy()
        w = wrench.wrench(k)
        xc = plant_step(oracle, xc, u0, p_true, w, dt, substeps)
        t = np.stack([(-u0[:, 0] + u0[:, 1] + u0[:, 3]), (-u0[:, 0] - u0[:, 1] - u0[:, 3]), (u0[:, 0] + u0[:, 1] - u0[:, 3]),
                      (u0[:, 0] - u0[:, 1] + u0[:, 3]), -u0[:, 2], -u0[:, 2]], axis=1) / rotor
        acc = (xc[:, 6:12] - vprev) / ekf.par.dt
        vprev = xc[:, 6:12].copy()
        _, mp, rc = ekf.update(xe, Pe, t, xc, acc)
        assert rc == 0
        if handoff:
            pfull[:, :, :4] = mp[:, None, :]
        log["u"].append(u0); log["x"].append(xc.copy()); log["status"].append(res["status"].copy()); log["wrench"].append(w)
        log["est"].append(xe[:, 12:].copy()); log["mpc_p"].append(mp.copy())
    return {k: np.array(v) for k, v in log.items()}
