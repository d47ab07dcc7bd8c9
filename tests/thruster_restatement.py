"""CPU restatement of the plant's thruster stage (include/bluerov2_nmpc.h, brov_thruster_*), the yardstick of thruster_eval_kernel and
plant_thruster_kernel in bluerov2_amd/csrc/plant_wrench.hip.  A helper, not collected.

Stage: for instance b at plant tick k, with t the six commands of the result record,
    c[i] = t[i] < lo[i] ? lo[i] : (t[i] > hi[i] ? hi[i] : t[i])                  (np.where: a NaN passes through)
    a[i] = k >= onset[b] ? gain[b][i] * c[i] + bias[b][i] : c[i]
    g[r] = ((((K[r][0]*a[0] + K[r][1]*a[1]) + K[r][2]*a[2]) + K[r][3]*a[3]) + K[r][4]*a[4]) + K[r][5]*a[5]
every operation one IEEE FP64 operation in this order: numpy elementwise `*` and `+` are separate operations and never contract.
Statistics of the plant steps: clip_ticks[b][i] += (t[i] outside its limits), lost_sq[b] += sum_i (t[i] - a[i])^2 -- six squares summed in
index order, then one add into the running sum --, last = a.

Plant: the step goes through slots the oracle already has and never through the device's thrust path: the input is ZERO, the stage's
forces enter as disturbances, p[0..3] + (g0, g1, g2, g5), and its roll / pitch moments as the 6-disturbance variant's drp = (g3, g4);
wrench_restatement.rk4_under_wrench integrates that under a world wrench (zeros: none)."""
import numpy as np

from wrench_restatement import rk4_under_wrench

ROTOR = 0.026546960744430276
# the model's own propulsion matrix (the reference's bluerov2.py:95-100)
K_MODEL = np.array([[0.707, 0.707, -0.707, -0.707, 0, 0],
                    [0.707, -0.707, 0.707, -0.707, 0, 0],
                    [0, 0, 0, 0, 1, 1],
                    [0, 0, 0, 0, 0, 0],
                    [0, 0, 0, 0, 0, 0],
                    [0.167, -0.167, -0.175, 0.175, 0, 0]], dtype=np.float64)


def allocation(u0):
    """the six commands of the result record from u0 [B][4], in the operation order of the device's epilogue"""
    u0 = np.asarray(u0, dtype=np.float64)
    return np.stack([((-u0[:, 0] + u0[:, 1]) + u0[:, 3]) / ROTOR, ((-u0[:, 0] + -u0[:, 1]) + -u0[:, 3]) / ROTOR,
                     ((u0[:, 0] + u0[:, 1]) + -u0[:, 3]) / ROTOR, ((u0[:, 0] + -u0[:, 1]) + u0[:, 3]) / ROTOR,
                     -u0[:, 2] / ROTOR, -u0[:, 2] / ROTOR], axis=1)


class ThrusterRestatement:
    def __init__(self, B, K=None, lo=None, hi=None, gain=None, bias=None, onset=None):
        self.B = int(B)
        self.K = K_MODEL.copy() if K is None else np.array(K, dtype=np.float64).reshape(6, 6)
        self.lo = np.broadcast_to(np.asarray(-np.inf if lo is None else lo, dtype=np.float64), (6,)).copy()
        self.hi = np.broadcast_to(np.asarray(np.inf if hi is None else hi, dtype=np.float64), (6,)).copy()
        self.gain = np.broadcast_to(np.asarray(1.0 if gain is None else gain, dtype=np.float64), (self.B, 6)).copy()
        self.bias = np.broadcast_to(np.asarray(0.0 if bias is None else bias, dtype=np.float64), (self.B, 6)).copy()
        self.onset = np.broadcast_to(np.asarray(0 if onset is None else onset, dtype=np.int64), (self.B,)).copy()
        self.reset_stats()

    def reset_stats(self):
        self.clip_ticks = np.zeros((self.B, 6), dtype=np.int32)
        self.lost_sq = np.zeros(self.B)
        self.last = np.zeros((self.B, 6))
        self.steps = 0

    def stage(self, k, t):
        """(applied a [B][6], wrench g [B][6]) for the commands t [B][6] at tick k; moves nothing"""
        t = np.asarray(t, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            c = np.where(t < self.lo, self.lo, np.where(t > self.hi, self.hi, t))
            f = self.gain * c
            f = f + self.bias
            a = np.where((int(k) >= self.onset)[:, None], f, c)
            g = np.empty((self.B, 6))
            for r in range(6):
                acc = self.K[r, 0] * a[:, 0] + self.K[r, 1] * a[:, 1]
                for i in range(2, 6):
                    acc = acc + self.K[r, i] * a[:, i]
                g[:, r] = acc
        return a, g

    def account(self, t, a):
        """what one plant step adds to the statistics"""
        t = np.asarray(t, dtype=np.float64)
        self.clip_ticks += ((t < self.lo) | (t > self.hi)).astype(np.int32)
        d = t - a
        sq = d * d
        s = sq[:, 0]
        for i in range(1, 6):
            s = s + sq[:, i]
        self.lost_sq = self.lost_sq + s
        self.last = a.copy()
        self.steps += 1

    def step(self, k, t):
        a, g = self.stage(k, t)
        self.account(t, a)
        return a, g


def plant_step(oracle, x, p, g, w=None, dt=0.05, substeps=1, prp=None):
    """batched restated plant step under the stage's wrench g [B][6] = [X Y Z K M N] (and a world wrench w [B][6], the 6-disturbance
    variant's moments prp [B][2] added to g3, g4): x [B][12], p [B][16]"""
    B = len(x)
    w = np.zeros((B, 6)) if w is None else w
    out = []
    for b in range(B):
        pa = np.array(p[b], dtype=np.float64, copy=True)
        pa[0] += g[b, 0]; pa[1] += g[b, 1]; pa[2] += g[b, 2]; pa[3] += g[b, 5]
        drp = np.array([g[b, 3], g[b, 4]]) + (0.0 if prp is None else prp[b])
        out.append(rk4_under_wrench(oracle, x[b], np.zeros(4), pa, w[b], dt, substeps, drp=drp))
    return np.stack(out)


def cpu_thruster_loop(oracle, ekf, thr, traj, x0, p_ctrl, p_true, N, ticks, line0=0, dt=0.05, substeps=1, handoff=True, wrench=None):
    """wrench_restatement.cpu_dob_loop with the thruster stage `thr` (a ThrusterRestatement) between the commands and the plant: window ->
    the oracle's RTI step -> thr.step at the tick -> the restated plant under its wrench (and wrench.wrench(k), if given) -> the oracle
    EKF fed with the COMMANDED thrusts -> hand-off (skipped with handoff=False; ekf=None: no observer at all).
    Returns dict(u, x [ticks+1], status, applied, est, mpc_p)."""
    from oracle import trajectory_oracle as T
    B = len(x0)
    op = oracle.opts(N, None)
    x, u, pi, lam = oracle.init_iterate(op, B)
    pfull = np.ascontiguousarray(np.broadcast_to(np.asarray(p_ctrl, dtype=np.float64).reshape(-1, 16)[:, None, :], (B, N + 1, 16)))
    xe, Pe = ekf.init_state(B) if ekf is not None else (None, None)
    xc = np.array(x0, dtype=np.float64, copy=True)
    vprev = np.zeros((B, 6))
    log = dict(u=[], x=[xc.copy()], status=[], applied=[], commanded=[], est=[], mpc_p=[])
    res = None
    for k in range(ticks):
        yref = np.ascontiguousarray(np.broadcast_to(T.window(traj, line0 + k, N), (B, N + 1, 16)))
        _, res = oracle.rti_step_batch(op, xc, yref, pfull, x, u, pi, lam, res_prev=res)
        u0 = res["u0"].copy()
        t = allocation(u0)
        a, g = thr.step(k, t)
        xc = plant_step(oracle, xc, p_true, g, None if wrench is None else wrench.wrench(k), dt, substeps)
        log["u"].append(u0); log["x"].append(xc.copy()); log["status"].append(res["status"].copy()); log["applied"].append(a)
        log["commanded"].append(t)
        if ekf is not None:
            acc = (xc[:, 6:12] - vprev) / ekf.par.dt
            vprev = xc[:, 6:12].copy()
            _, mp, rc = ekf.update(xe, Pe, t, xc, acc)
            assert rc == 0
            if handoff:
                pfull[:, :, :4] = mp[:, None, :]
            log["est"].append(xe[:, 12:].copy()); log["mpc_p"].append(mp.copy())
    return {k: np.array(v) for k, v in log.items()}
