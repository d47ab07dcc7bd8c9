"""CPU restatement of the plant's delay stage (include/bluerov2_nmpc.h, brov_delay_*), the yardstick of delay_shift_kernel and
delay_predict_kernel in bluerov2_amd/csrc/delay_kernel.hip.  A helper, not collected.

Queue: per instance a ring of the last D commanded records (u0[4] | thrust[6]), D = max(max_b delay[b], comp) + 1, zero-filled, indexed by
the stage's own step count n.  Step n with the commanded record c(n):
    a(n) = delay[b] == 0 ? c(n) : (n < delay[b] ? 0 : ring[(n - delay[b]) mod D])         read first
    ring[n mod D] = c(n)
Copies only: the device agrees bit for bit.

Predictor: x^ = Phi(... Phi(Phi(y, c(n - comp)), c(n - comp + 1)) ..., c(n - 1)), Phi = the oracle's one RK4 step over dt_pred with the
controller's stage-0 parameters (and the 6-disturbance variant's moments), the inputs the queue's u0, zeros for steps before the first."""
import numpy as np

from thruster_restatement import allocation
from thruster_restatement import plant_step as plant_step_thrusters

DELAY_MAX = 8


class DelayRestatement:
    def __init__(self, B, delay=None, comp=0):
        self.B = int(B)
        self.delay = np.broadcast_to(np.asarray(0 if delay is None else delay, dtype=np.int64), (self.B,)).copy()
        self.comp = int(comp)
        assert self.delay.min() >= 0 and self.delay.max() <= DELAY_MAX and 0 <= self.comp <= DELAY_MAX
        self.D = max(int(self.delay.max()), self.comp) + 1
        self.reset()

    def reset(self):
        self.ring = np.zeros((self.B, self.D, 10))
        self.last = np.zeros((self.B, 10))
        self.n = 0

    def step(self, u0, thrust):
        """one step of the stage with the commanded u0 [B][4] and thrust [B][6]: returns the applied (u0 [B][4], thrust [B][6])"""
        c = np.concatenate([np.asarray(u0, dtype=np.float64).reshape(self.B, 4), np.asarray(thrust, dtype=np.float64).reshape(self.B, 6)], axis=1)
        a = np.empty((self.B, 10))
        for b in range(self.B):
            d = int(self.delay[b])
            a[b] = c[b] if d == 0 else (0.0 if self.n < d else self.ring[b, (self.n - d) % self.D])
        self.ring[:, self.n % self.D] = c
        self.last = a
        self.n += 1
        return a[:, :4].copy(), a[:, 4:].copy()

    def record(self, step):
        """[B][10]: the commanded record of `step` (one of the last D), zeros for a step before the first"""
        assert self.n - self.D <= step < self.n
        return np.zeros((self.B, 10)) if step < 0 else self.ring[:, step % self.D].copy()

    def queue(self):
        """[B][D][4]: the u0 of the last D commanded records, oldest first"""
        return np.stack([self.record(self.n - self.D + i)[:, :4] for i in range(self.D)], axis=1)

    def predictor_inputs(self):
        """[comp][B][4]: the inputs the predictor integrates through, oldest first"""
        return np.stack([self.record(self.n - self.comp + i)[:, :4] for i in range(self.comp)]) if self.comp else np.zeros((0, self.B, 4))

    def predict(self, oracle, y, p0, dt_pred, drp=None):
        """x^ [B][12] from y [B][12] with the stage-0 parameters p0 [B][16] (drp [B][2]: the 6-disturbance variant's moments)"""
        x = np.array(y, dtype=np.float64, copy=True)
        for u in self.predictor_inputs():
            x = np.stack([oracle.rk4(x[b], u[b], p0[b], dt_pred, None if drp is None else drp[b]) for b in range(self.B)])
        return x


def rms_position_error(x_log, traj, line0=0):
    """RMS over ticks and instances of |position after tick k - row line0 + k + 1|"""
    ticks = len(x_log) - 1
    err = x_log[1:, :, :3] - traj[line0 + 1:line0 + ticks + 1, None, :3]
    return float(np.sqrt((err ** 2).sum(-1).mean()))


def cpu_delay_loop(oracle, dl, traj, x0, p_ctrl, p_true, N, ticks, line0=0, dt=0.05, substeps=1, dt_pred=None, thr=None, ekf=None,
                   observer_applied=False):
    """The closed loop behind the delay stage `dl` (a DelayRestatement) on the CPU, tick for tick what brov_closed_loop / _dob enqueue:
    predictor from the plant's state -> window(line0 + k + comp) -> the oracle's RTI step from x^ -> dl.step -> the restated plant with the
    APPLIED record (thr, a ThrusterRestatement: behind that stage, at tick k; else the oracle's RK4 with the applied u0) -> with `ekf` (an
    EkfOracle) the observer fed with the commanded thrusts (observer_applied: the applied ones) and its hand-off.
    A loop whose state turns non-finite ends behind that tick.  Returns dict(u [ticks][B][4] commanded, x [ticks+1][B][12], status, applied_u, applied_t, xhat, est, mpc_p)."""
    from oracle import trajectory_oracle as T
    B = len(x0)
    op = oracle.opts(N, None)
    dt_pred = op.Ts if dt_pred is None else dt_pred
    x, u, pi, lam = oracle.init_iterate(op, B)
    pfull = np.ascontiguousarray(np.broadcast_to(np.asarray(p_ctrl, dtype=np.float64).reshape(-1, 16)[:, None, :], (B, N + 1, 16)))
    xe, Pe = ekf.init_state(B) if ekf is not None else (None, None)
    xc = np.array(x0, dtype=np.float64, copy=True)
    vprev = np.zeros((B, 6))
    log = dict(u=[], x=[xc.copy()], status=[], applied_u=[], applied_t=[], xhat=[], est=[], mpc_p=[])
    res = None
    for k in range(ticks):
        if not np.isfinite(xc).all():      # a loop that has diverged ends here: the logs hold the ticks that ran, the last state is the culprit
            break
        xhat = dl.predict(oracle, xc, pfull[:, 0], dt_pred)
        yref = np.ascontiguousarray(np.broadcast_to(T.window(traj, line0 + k + dl.comp, N), (B, N + 1, 16)))
        _, res = oracle.rti_step_batch(op, xhat, yref, pfull, x, u, pi, lam, res_prev=res)
        u0 = res["u0"].copy()
        t = allocation(u0)
        au, at = dl.step(u0, t)
        if thr is not None:
            xc = plant_step_thrusters(oracle, xc, p_true, thr.step(k, at)[1], None, dt, substeps)
        else:
            for _ in range(substeps):
                xc = np.stack([oracle.rk4(xc[b], au[b], p_true[b], dt / substeps) for b in range(B)])
        log["u"].append(u0); log["x"].append(xc.copy()); log["status"].append(res["status"].copy())
        log["applied_u"].append(au); log["applied_t"].append(at); log["xhat"].append(xhat)
        if ekf is not None:
            acc = (xc[:, 6:12] - vprev) / ekf.par.dt
            vprev = xc[:, 6:12].copy()
            _, mp, rc = ekf.update(xe, Pe, at if observer_applied else t, xc, acc)
            assert rc == 0
            pfull[:, :, :4] = mp[:, None, :]
            log["est"].append(xe[:, 12:].copy()); log["mpc_p"].append(mp.copy())
    return {k: np.array(v) for k, v in log.items()}
