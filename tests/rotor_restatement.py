"""CPU restatement of the plant's rotor stage (include/bluerov2_nmpc.h, brov_rotor_*), the yardstick of rotor_shift_kernel and
rotor_eval_kernel in bluerov2_amd/csrc/rotor_kernel.hip.  A helper, not collected.

Per instance b and thruster i, with the state r (zero at set or reset), the command t and the coefficients alpha, beta -- which are GIVEN
(the stage's, rotor_coeffs() of the package or BatchSolver.rotor_coeffs()); nothing here calls exp --, every operation rounded on its own:
    c  = t < lo[i] ? lo[i] : (t > hi[i] ? hi[i] : t)
    if !isfinite(c): c = r
    d  = r + (-c)
    m  = c + beta  * d          the mean thrust over the step, what the plant is given
    r' = c + alpha * d          the state at the end of the step
a pair (alpha, beta) == (0, 0), the pair of tau = 0, copies m = r' = c.  The applied u0 is the allocation's left inverse of m:
    u0[0] = (rc * (((-m0 + -m1) +  m2) +  m3)) * 0.25        u0[1] = (rc * ((( m0 + -m1) +  m2) + -m3)) * 0.25
    u0[3] = (rc * ((( m0 + -m1) + -m2) +  m3)) * 0.25        u0[2] = -((rc * (m4 + m5)) * 0.5)
except for an instance whose six pairs are (0, 0) and whose six c have the bits of their t: it keeps the u0 it was given.
lag_sq += sum_i (c_i - m_i)^2: six squares summed in index order, then one add."""
import numpy as np

from thruster_restatement import ROTOR, allocation


def pinv_allocation(m):
    """u0 [B][4] from the thrusts m [B][6], in the operation order of rotor_shift_kernel"""
    m = np.asarray(m, dtype=np.float64)
    m0, m1, m2, m3, m4, m5 = (m[:, i] for i in range(6))
    u = np.empty((len(m), 4))
    u[:, 0] = (ROTOR * (((-m0 + -m1) + m2) + m3)) * 0.25
    u[:, 1] = (ROTOR * (((m0 + -m1) + m2) + -m3)) * 0.25
    u[:, 3] = (ROTOR * (((m0 + -m1) + -m2) + m3)) * 0.25
    u[:, 2] = -((ROTOR * (m4 + m5)) * 0.5)
    return u


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class RotorRestatement:
    def __init__(self, B, alpha, beta, lo=None, hi=None):
        self.B = int(B)
        self.alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (self.B, 6)).copy()
        self.beta = np.broadcast_to(np.asarray(beta, dtype=np.float64), (self.B, 6)).copy()
        self.lo = np.broadcast_to(np.asarray(-np.inf if lo is None else lo, dtype=np.float64), (6,)).copy()
        self.hi = np.broadcast_to(np.asarray(np.inf if hi is None else hi, dtype=np.float64), (6,)).copy()
        self.reset()

    def reset(self):
        self.r = np.zeros((self.B, 6))
        self.last = np.zeros((self.B, 6))
        self.last_u0 = np.zeros((self.B, 4))
        self.lag_sq = np.zeros(self.B)
        self.steps = 0

    def stage(self, t, r=None):
        """(c, m, r', untouched [B]) for the commands t [B][6] from the state r [B][6] (None: the stage's own); moves nothing"""
        t = np.asarray(t, dtype=np.float64).reshape(self.B, 6)
        r = self.r if r is None else np.asarray(r, dtype=np.float64).reshape(self.B, 6)
        with np.errstate(invalid="ignore", over="ignore"):
            c = np.where(t < self.lo, self.lo, np.where(t > self.hi, self.hi, t))
            c = np.where(np.isfinite(c), c, r)
            copy = (self.alpha == 0.0) & (self.beta == 0.0)
            d = r + (-c)
            bd = self.beta * d
            ad = self.alpha * d
            m = np.where(copy, c, c + bd)
            rn = np.where(copy, c, c + ad)
        untouched = (copy & (_bits(c) == _bits(t))).all(axis=1)
        return c, m, rn, untouched

    def eval(self, t, r=None):
        """(applied [B][6], new state [B][6]): what rotor_eval_kernel returns"""
        _, m, rn, _ = self.stage(t, r)
        return m, rn

    def step(self, u0, thrust):
        """one step of the stage with the record's u0 [B][4] and thrust [B][6]: returns the applied (u0 [B][4], thrust [B][6])"""
        u0 = np.asarray(u0, dtype=np.float64).reshape(self.B, 4)
        c, m, rn, untouched = self.stage(thrust)
        d = c + (-m)
        sq = d * d
        s = sq[:, 0]
        for i in range(1, 6):
            s = s + sq[:, i]
        self.lag_sq = self.lag_sq + s
        self.r = rn
        self.last = m.copy()
        self.last_u0 = np.where(untouched[:, None], u0, pinv_allocation(m))
        self.steps += 1
        return self.last_u0.copy(), m.copy()


def cpu_rotor_loop(oracle, ro, traj, x0, p_ctrl, p_true, N, ticks, line0=0, dt=0.05):
    """The closed loop behind the rotor stage `ro` (a RotorRestatement whose coefficients hold for dt) on the CPU, tick for tick what
    brov_closed_loop enqueues: window(line0 + k) -> the oracle's RTI step from the plant's state -> the allocation of u0 -> ro.step -> the
    oracle's RK4 with the APPLIED u0.  Returns dict(u [ticks][B][4] commanded, x [ticks+1][B][12], status, applied_u, applied_t)."""
    from oracle import trajectory_oracle as T
    B = len(x0)
    op = oracle.opts(N, None)
    x, u, pi, lam = oracle.init_iterate(op, B)
    pfull = np.ascontiguousarray(np.broadcast_to(np.asarray(p_ctrl, dtype=np.float64).reshape(-1, 16)[:, None, :], (B, N + 1, 16)))
    xc = np.array(x0, dtype=np.float64, copy=True)
    log = dict(u=[], x=[xc.copy()], status=[], applied_u=[], applied_t=[])
    res = None
    for k in range(ticks):
        yref = np.ascontiguousarray(np.broadcast_to(T.window(traj, line0 + k, N), (B, N + 1, 16)))
        _, res = oracle.rti_step_batch(op, xc, yref, pfull, x, u, pi, lam, res_prev=res)
        u0 = res["u0"].copy()
        au, at = ro.step(u0, allocation(u0))
        xc = np.stack([oracle.rk4(xc[b], au[b], p_true[b], dt) for b in range(B)])
        log["u"].append(u0); log["x"].append(xc.copy()); log["status"].append(res["status"].copy())
        log["applied_u"].append(au); log["applied_t"].append(at)
    return {k: np.array(v) for k, v in log.items()}
