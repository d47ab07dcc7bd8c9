"""CPU restatement of the reference's RLS-FF estimator BLUEROV2_AMPC::RLSFF() (bluerov2_dobmpc/src/bluerov2_ampc.cpp:731-1046),
the yardstick of the batched HIP kernel (bluerov2_amd/csrc/rls_kernel.hip, brov_rls_*).

Vectorised across instances (and the four axes X, Y, Z, N) only: every operation is elementwise IEEE FP64 in the order the
reference writes it -- dot products and matrix-vector products summed sequentially in index order, std::accumulate from 0.0 over
the window oldest to newest, the variance as sum (v - mean)^2 from 0.0 then / size, the gain by division, P updated as
(P - (K x^T) P) / lambda with the product associated left to right.  No np.sum / np.mean / @ / np.dot: pairwise summation and
BLAS FMAs would not be bit-identical to it.  Checked by reading against the reference's source (Eigen and ROS are not here).

Axis a of instance b at tick k:  x = [acc, v, 1, v|v|],  y = esti_x(12 | 13 | 14 | 17),  e = y - x.theta,  F = var_short / var_long,
lambda -/+ step with clamps, K = P x / (lambda + x.(P x)),  theta += K e,  P = (P - (K x^T) P) / lambda.
"""
import numpy as np

# branch codes of the forgetting-factor update, per (instance, axis) and tick
LAM_DOWN, LAM_FLOOR, LAM_UP, LAM_CEIL = 0, 1, 2, 3


class RlsffRestatement:
    def __init__(self, B, n_short=5, n_long=50, threshold=0.8, lambda_step=0.01, lambda_min=0.5, lambda_max=1.0, lambda0=0.9,
                 p0=1.0, compensate_coef=0.032546960744430276, rotor_constant=0.026546960744430276):
        self.B = B
        self.ns, self.nl = n_short, n_long
        self.thr, self.step_, self.lmin, self.lmax, self.l0, self.p0 = threshold, lambda_step, lambda_min, lambda_max, lambda0, p0
        self.cc, self.rc = compensate_coef, rotor_constant
        self.reset()

    @classmethod
    def from_params(cls, B, p):
        return cls(B, p.n_short, p.n_long, p.threshold, p.lambda_step, p.lambda_min, p.lambda_max, p.lambda0, p.p0, p.compensate_coef,
                   p.rotor_constant)

    def reset(self):
        B = self.B
        self.theta = np.zeros((B, 4, 4))                      # [instance][axis][component]
        self.P = np.zeros((B, 4, 4, 4))
        for i in range(4):
            self.P[:, :, i, i] = self.p0
        self.lam = np.full((B, 4), self.l0)
        self.F = np.zeros((B, 4))
        self.e = np.zeros((B, 4))
        self.win_s, self.win_l = [], []                        # lists of [B][4] error arrays, oldest first
        self.wf = np.zeros((B, 6))

    def set_state(self, theta=None, P=None, lam=None):
        if theta is not None:
            self.theta = np.array(theta, dtype=np.float64).reshape(self.B, 4, 4)
        if P is not None:
            self.P = np.array(P, dtype=np.float64).reshape(self.B, 4, 4, 4)
        if lam is not None:
            self.lam = np.array(lam, dtype=np.float64).reshape(self.B, 4)
        self.win_s, self.win_l = [], []

    @staticmethod
    def _window_var(win):
        s = np.zeros_like(win[0])
        for v in win:
            s = s + v
        mean = s / float(len(win))
        var = np.zeros_like(win[0])
        for v in win:
            d = v - mean
            var = var + d * d
        return var / float(len(win))

    def step(self, y, acc, vel, rpy):
        """one tick; y / acc / vel [B][4] (axes X, Y, Z, N), rpy [B][3].  Returns the lambda branch codes [B][4]."""
        y, acc, vel, rpy = (np.asarray(a, dtype=np.float64) for a in (y, acc, vel, rpy))
        th, P = self.theta, self.P
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            x = [acc, vel, np.ones_like(vel), vel * np.abs(vel)]
            xt = x[0] * th[:, :, 0]
            for j in range(1, 4):
                xt = xt + x[j] * th[:, :, j]
            e = y - xt
            self.win_s.append(e)
            self.win_l.append(e)
            if len(self.win_s) > self.ns:
                self.win_s.pop(0)
            if len(self.win_l) > self.nl:
                self.win_l.pop(0)
            F = self._window_var(self.win_s) / self._window_var(self.win_l)
            lam = self.lam
            down = F > self.thr
            dn, up = lam - self.step_, lam + self.step_
            code = np.where(down, np.where(dn >= self.lmin, LAM_DOWN, LAM_FLOOR), np.where(up <= self.lmax, LAM_UP, LAM_CEIL))
            lam = np.where(down, np.where(dn >= self.lmin, dn, self.lmin), np.where(up <= self.lmax, up, self.lmax))
            Px = []
            for i in range(4):
                s = P[:, :, i, 0] * x[0]
                for j in range(1, 4):
                    s = s + P[:, :, i, j] * x[j]
                Px.append(s)
            xPx = x[0] * Px[0]
            for j in range(1, 4):
                xPx = xPx + x[j] * Px[j]
            den = lam + xPx
            K = [Px[i] / den for i in range(4)]
            thn = np.empty_like(th)
            for i in range(4):
                thn[:, :, i] = th[:, :, i] + K[i] * e
            Pn = np.empty_like(P)
            for i in range(4):
                M = [K[i] * x[j] for j in range(4)]
                for j in range(4):
                    s = M[0] * P[:, :, 0, j]
                    for k in range(1, 4):
                        s = s + M[k] * P[:, :, k, j]
                    Pn[:, :, i, j] = (P[:, :, i, j] - s) / lam
        self.theta, self.P, self.lam, self.F, self.e = thn, Pn, lam, F, e
        self.wf = self.wf_env(rpy)
        return code

    def wf_env(self, rpy):
        """world-frame environmental disturbance from theta(2) (bluerov2_ampc.cpp:1000-1005, rows 4-6 as written there)"""
        phi, the, psi = rpy[:, 0], rpy[:, 1], rpy[:, 2]
        tX, tY, tZ, tN = (self.theta[:, a, 2] for a in range(4))
        cf, sf, ct, st, cp, sp = np.cos(phi), np.sin(phi), np.cos(the), np.sin(the), np.cos(psi), np.sin(psi)
        with np.errstate(invalid="ignore", over="ignore"):
            return np.stack([(cp * ct) * tX + (-sp * cf + cp * st * sf) * tY + (sp * sf + cp * cf * st) * tZ,
                             (sp * ct) * tX + (cp * cf + sf * st * sp) * tY + (-cp * sf + st * sp * cf) * tZ,
                             (-st) * tX + (ct * sf) * tY + (ct * cf) * tZ,
                             cf * st / ct * tN,
                             (sf) * tN,
                             (cf / ct) * tN], axis=1)

    def mpc_p(self):
        """AMPC's hand-off p[0..3] (bluerov2_ampc.cpp:346-349)"""
        t2 = self.theta[:, :, 2]
        return np.stack([t2[:, 0] / self.cc, t2[:, 1] / self.cc, t2[:, 2] / self.rc, t2[:, 3] / self.rc], axis=1)

    def status(self):
        fin = np.isfinite(self.theta).all(axis=(1, 2)) & np.isfinite(self.P).all(axis=(1, 2, 3))
        return np.where(fin, 0, 2).astype(np.int32)
