"""CPU restatement of the plant's thrust-curve stage (include/bluerov2_nmpc_curve.h, brov_curve_*), the yardstick of curve_shift_kernel<PART> and
curve_eval_kernel in bluerov2_amd/csrc/curve_kernel.hip.  A helper, not collected.

Per instance b and thruster i, t = thrust[i] of the record received, every operation rounded on its own (numpy's element-wise products and
sums are), nothing here divides: the slopes of the tables and inv_quantum are GIVEN (the stage's own, BatchSolver.thrust_curve_table(), or
table_slopes() / 1.0 / quantum, which are the host's expressions).
    COMMAND   w = t | (((p0 t + p1) t + p2) t + p3) t + p4 | lookup(pre, t);   quantum > 0: w = quantum * rint(w * inv_quantum)
    THRUST    f = w | k * (w * |w|) | kl * (v + (-dl)) for v <= dl, kr * (v + (-dr)) for v >= dr, +0.0 between, v = w * |w| | lookup(curve, w)
              f = eff * f unless eff == 1.0
    lookup    w <= x[0]: y[0];  w >= x[K-1]: y[K-1];  else y[j] + slope[j] * (w + (-x[j])), j the largest index with x[j] <= w
    NaN       a NaN that enters a part leaves it with its bits; a NaN a part makes of another input is 0x7FF8000000000000
A part that changes a bit of the six values writes u0 = the allocation's left inverse of its output (rotor_restatement.pinv_allocation), else
the record passes whole; BOTH is COMMAND then THRUST.  err_sq += sum_i (wanted_i - f_i)^2: six squares summed in index order, then one add;
dead_ticks += (f == 0 and wanted != 0); charge += dt * sum_i amps_i with an amps column."""
import numpy as np

from rotor_restatement import pinv_allocation

LINEAR, BASIC, DEADZONE, TABLE = 0, 1, 2, 3
PRE_NONE, PRE_POLY, PRE_TABLE = 0, 1, 2
QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def table_slopes(x, y):
    """the host's slopes: (y[j+1] - y[j]) / (x[j+1] - x[j]) in doubles, slope[K-1] = 0"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    s = np.zeros(len(x))
    s[:-1] = (y[1:] - y[:-1]) / (x[1:] - x[:-1])
    return s


def nan_rule(out, inp):
    return np.where(np.isnan(inp), inp, np.where(np.isnan(out), QNAN, out))


def lookup(x, y, slope, w):
    """the stage's lookup of w (any shape) in the table (x, y, slope); a NaN w gives a NaN (the caller's nan_rule makes it w)"""
    x, y, slope = (np.asarray(a, dtype=np.float64) for a in (x, y, slope))
    w = np.asarray(w, dtype=np.float64)
    K = len(x)
    with np.errstate(invalid="ignore", over="ignore"):
        j = np.clip(np.searchsorted(x, np.where(np.isnan(w), x[0], w), side="right") - 1, 0, K - 1)
        v = y[j] + slope[j] * (w + (-x[j]))
        v = np.where(w <= x[0], y[0], np.where(w >= x[K - 1], y[K - 1], v))
    return v


class CurveRestatement:
    def __init__(self, B, kind=LINEAR, pre=PRE_NONE, quantum=0.0, k=1.0, kl=1.0, kr=1.0, dl=0.0, dr=0.0, pre_poly=(0.0, 0.0, 0.0, 1.0, 0.0), eff=1.0,
                 curve=None, pre_table=None):
        """curve: dict(x, y, slope[, amps, amps_slope]) (amps: None or absent for no column); pre_table: dict(x, y, slope)"""
        self.B = int(B)
        self.kind, self.pre = int(kind), int(pre)
        self.quantum = float(quantum)
        self.inv_quantum = 1.0 / self.quantum if self.quantum > 0.0 else 0.0
        self.k, self.kl, self.kr, self.dl, self.dr = float(k), float(kl), float(kr), float(dl), float(dr)
        self.pre_poly = np.asarray(pre_poly, dtype=np.float64).copy()
        self.eff = np.broadcast_to(np.asarray(eff, dtype=np.float64), (self.B, 6)).copy()
        self.curve, self.pre_table = curve, pre_table
        self.has_amps = self.kind == TABLE and curve is not None and curve.get("amps") is not None
        self.reset()

    def reset(self):
        self.wanted = np.zeros((self.B, 6))
        self.last_command = np.zeros((self.B, 6))
        self.last_thrust = np.zeros((self.B, 6))
        self.last_u0 = np.zeros((self.B, 4))
        self.err_sq = np.zeros(self.B)
        self.dead_ticks = np.zeros((self.B, 6), dtype=np.int32)
        self.charge = np.zeros(self.B)
        self.steps = 0

    # ---- the two parts on values of any shape [..., 6] -----------------------------------------------------------------------------------------
    def command(self, t):
        t = np.asarray(t, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            if self.pre == PRE_POLY:
                w = np.full(t.shape, self.pre_poly[0])
                for i in range(1, 5):
                    w = w * t
                    w = w + self.pre_poly[i]
            elif self.pre == PRE_TABLE:
                w = lookup(self.pre_table["x"], self.pre_table["y"], self.pre_table["slope"], t)
            else:
                w = t.copy()
            if self.quantum > 0.0:
                w = w * self.inv_quantum
                w = self.quantum * np.rint(w)
        return nan_rule(w, t)

    def thrust(self, w, eff=None):
        """(f, amps): amps zeros without a column"""
        w = np.asarray(w, dtype=np.float64)
        eff = self.eff if eff is None else eff
        amps = np.zeros(w.shape)
        with np.errstate(invalid="ignore", over="ignore"):
            if self.kind == BASIC:
                f = w * np.abs(w)
                f = self.k * f
            elif self.kind == DEADZONE:
                v = w * np.abs(w)
                f = np.where(v <= self.dl, self.kl * (v + (-self.dl)), np.where(v >= self.dr, self.kr * (v + (-self.dr)), 0.0))
            elif self.kind == TABLE:
                f = lookup(self.curve["x"], self.curve["y"], self.curve["slope"], w)
                if self.has_amps:
                    amps = nan_rule(lookup(self.curve["x"], self.curve["amps"], self.curve["amps_slope"], w), w)
            else:
                f = w.copy()
            f = np.where(eff == 1.0, f, eff * f)
        return nan_rule(f, w), amps

    def eval(self, values, part="both"):
        """(out [B][6], amps [B][6]): what curve_eval_kernel returns"""
        v = np.asarray(values, dtype=np.float64).reshape(self.B, 6)
        a = np.zeros((self.B, 6))
        if part in ("command", "both"):
            v = self.command(v)
        if part in ("thrust", "both"):
            v, a = self.thrust(v)
        return v, a

    # ---- the parts on records, with the books --------------------------------------------------------------------------------------------------
    def step_command(self, u0, thrust):
        """the COMMAND launch: returns the applied (u0 [B][4], thrust [B][6])"""
        u0 = np.asarray(u0, dtype=np.float64).reshape(self.B, 4)
        t = np.asarray(thrust, dtype=np.float64).reshape(self.B, 6)
        w = self.command(t)
        self.wanted, self.last_command = t.copy(), w.copy()
        changed = (_bits(w) != _bits(t)).any(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.where(changed[:, None], pinv_allocation(w), u0), w.copy()

    def step_thrust(self, u0, thrust, dt):
        """the THRUST launch on the record that arrives (the rotor stage's, or step_command's)"""
        u0 = np.asarray(u0, dtype=np.float64).reshape(self.B, 4)
        w = np.asarray(thrust, dtype=np.float64).reshape(self.B, 6)
        f, amps = self.thrust(w)
        self.last_thrust = f.copy()
        with np.errstate(invalid="ignore", over="ignore"):
            d = self.wanted + (-f)
            sq = d * d
            s, a = sq[:, 0], amps[:, 0]
            for i in range(1, 6):
                s = s + sq[:, i]
                a = a + amps[:, i]
            self.err_sq = self.err_sq + s
            if self.has_amps:
                self.charge = self.charge + dt * a
        self.dead_ticks = self.dead_ticks + ((f == 0.0) & (self.wanted != 0.0)).astype(np.int32)
        changed = (_bits(f) != _bits(w)).any(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            self.last_u0 = np.where(changed[:, None], pinv_allocation(f), u0)
        self.steps += 1
        return self.last_u0.copy(), f.copy()

    def step_both(self, u0, thrust, dt):
        """the BOTH launch: COMMAND followed by THRUST"""
        cu, ct = self.step_command(u0, thrust)
        return self.step_thrust(cu, ct, dt)


def cpu_curve_loop(oracle, cv, traj, x0, p_ctrl, p_true, N, ticks, line0=0, dt=0.05, ro=None, ekf=None, handoff=True):
    """The closed loop behind the thrust-curve stage `cv` (a CurveRestatement) on the CPU, tick for tick what brov_closed_loop / _dob enqueue:
    window(line0 + k) -> the oracle's RTI step from the plant's state -> the allocation of u0 -> cv (with `ro`, a RotorRestatement whose
    coefficients hold for dt: COMMAND, ro.step, THRUST; else BOTH) -> the oracle's RK4 with the APPLIED u0 -> with `ekf` (an EkfOracle) the
    observer fed the COMMANDED thrusts and, with handoff, its estimate into the controller's parameters.
    Returns dict(u [ticks][B][4] commanded, x [ticks+1][B][12], status, applied_u, applied_t, rotor_from [ticks][B][6], rotor_cmd, ekf_failed)."""
    from oracle import trajectory_oracle as T
    from thruster_restatement import allocation
    B = len(x0)
    op = oracle.opts(N, None)
    x, u, pi, lam = oracle.init_iterate(op, B)
    pfull = np.ascontiguousarray(np.broadcast_to(np.asarray(p_ctrl, dtype=np.float64).reshape(-1, 16)[:, None, :], (B, N + 1, 16)))
    xe, Pe = ekf.init_state(B) if ekf is not None else (None, None)
    xc = np.array(x0, dtype=np.float64, copy=True)
    vprev = np.zeros((B, 6))
    log = dict(u=[], x=[xc.copy()], status=[], applied_u=[], applied_t=[], rotor_from=[], rotor_cmd=[])
    res, ekf_failed = None, -1
    for k in range(ticks):
        yref = np.ascontiguousarray(np.broadcast_to(T.window(traj, line0 + k, N), (B, N + 1, 16)))
        _, res = oracle.rti_step_batch(op, xc, yref, pfull, x, u, pi, lam, res_prev=res)
        u0 = res["u0"].copy()
        t = allocation(u0)
        if ro is None:
            au, at = cv.step_both(u0, t, dt)
        else:
            cu, ct = cv.step_command(u0, t)
            log["rotor_from"].append(ro.r.copy()); log["rotor_cmd"].append(ro.stage(ct)[0])
            ru, rt = ro.step(cu, ct)
            au, at = cv.step_thrust(ru, rt, dt)
        xc = np.stack([oracle.rk4(xc[b], au[b], p_true[b], dt) for b in range(B)])
        log["u"].append(u0); log["x"].append(xc.copy()); log["status"].append(res["status"].copy())
        log["applied_u"].append(au); log["applied_t"].append(at)
        if ekf is not None:
            acc = (xc[:, 6:12] - vprev) / ekf.par.dt
            vprev = xc[:, 6:12].copy()
            _, mp, rc = ekf.update(xe, Pe, t, xc, acc)
            if rc != 0:                      # the observer gave up (a state that is not finite): the loop goes on without it
                ekf_failed, ekf = k, None
                continue
            if handoff:
                pfull[:, :, :4] = mp[:, None, :]
    out = {k: np.array(v) for k, v in log.items()}
    out["ekf_failed"] = ekf_failed           # the tick at which the observer gave up, -1: never
    return out
