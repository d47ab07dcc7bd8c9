"""One tick of the EKF disturbance observer in far more than double precision: the yardstick of tests/test_ekf_exact_cpu.py and
tests/test_gpu_ekf_exact.py (fixture tests/golden/ekf_exact.npz, scripts/make_ekf_exact_golden.py).

What the reference is.  The SAME algorithm as include/bluerov2_nmpc.h (brov_ekf_*) and test_oracle_ekf.np_update state it, carried out
in exact arithmetic (mpmath, 60 digits) -- the truncation error of the forward differences INCLUDED: F and H are the forward differences
of the RK4 map at x and of h at x_pred with the parameter fd_step, not the analytic Jacobians.  It is written from the formulas of the
numpy restatement (np_f, np_rk4, np_h, np_fd, np_update), not from the C oracle and not from the kernel:

    tau = K thrust;  the RK4 with its third stage at x + k2 / 3;  F = fd(rk4, x), x_pred = rk4(x), P_pred = F P F' + diag(Q);
    H = fd(h, x_pred);  S = H P_pred H' + R I;  Kal = P_pred H' S^-1;  x_new = x_pred + Kal (y - h(x_pred));
    P_new = (I - Kal H) P_pred (I - Kal H)' + R Kal Kal'   (Joseph form);
    wf = the estimated disturbance turned into the world frame with the MEASURED attitude;  mpc_p = its four entries, scaled.

Every input is taken as the exact value of the double it is given as, the filter's parameters too (a brov_ekf_params holds doubles);
the mass matrix is inverted exactly and its diagonal used, as the restatement does.  S is eliminated without row exchanges and the
pivots are returned: if one is not positive the tick's result is the prediction (x_pred, P_pred) and status is 1 -- the contract of
status 1 in the header -- else status is 0.  A chain of ticks can carry its state at 60 digits (tick() takes and returns mpf).
"""
import numpy as np

N = 18
DIGITS = 60
PAR_FIELDS = (("dt", 1), ("mass", 1), ("Ix", 1), ("Iy", 1), ("Iz", 1), ("ZG", 1), ("g", 1), ("bouyancy", 1), ("added_mass", 6), ("Dl", 6),
              ("Dnl", 6), ("K", 36), ("Q", 18), ("R", 1), ("fd_step", 1), ("compensate_coef", 1), ("rotor_constant", 1))
NPAR = sum(n for _, n in PAR_FIELDS)
IU = np.triu_indices(N)


def par_vector(par):
    """the fields of a brov_ekf_params (bluerov2_amd.EkfParams, the oracle's OrcEkfPar: the same names) as one vector"""
    return np.concatenate([np.atleast_1d(np.array(getattr(par, f), dtype=np.float64)) for f, _ in PAR_FIELDS])


def par_apply(par, vec):
    """... and back into such a structure (in place; the oracle's derived fields are the caller's to refresh)"""
    vec = np.asarray(vec, dtype=np.float64)
    assert vec.shape == (NPAR,)
    o = 0
    for f, n in PAR_FIELDS:
        if n == 1:
            setattr(par, f, float(vec[o]))
        else:
            a = getattr(par, f)
            for j in range(n):
                a[j] = float(vec[o + j])
        o += n
    return par


def par_dict(vec):
    o, d = 0, {}
    for f, n in PAR_FIELDS:
        d[f] = float(vec[o]) if n == 1 else np.array(vec[o:o + n], dtype=np.float64)
        o += n
    return d


def to_triu(P):
    return np.asarray(P)[..., IU[0], IU[1]]


def from_triu(v):
    v = np.asarray(v)
    P = np.zeros(v.shape[:-1] + (N, N))
    P[..., IU[0], IU[1]] = v
    P[..., IU[1], IU[0]] = v
    return P


def err_x(got, ref):
    """|got - ref| / max(1, |ref|), the worst entry of each filter (NaN where got is NaN); also for wf and mpc_p"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max(axis=-1)


def err_P(got, ref):
    """|got - ref| / max |ref| per filter, the worst entry of each"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return (np.abs(got - ref).max(axis=(-2, -1))) / np.abs(ref).max(axis=(-2, -1))


def np_outputs(p, xn, y12):
    """wf [6] and mpc_p [4] of an estimate in plain numpy (the formulas test_oracle_ekf.test_update_vs_numpy checks the oracle's against)"""
    phi, th, psi = y12[3:6]
    s, c = np.sin, np.cos
    Rz = np.array([[c(psi) * c(th), -s(psi) * c(phi) + c(psi) * s(th) * s(phi), s(psi) * s(phi) + c(psi) * c(phi) * s(th)],
                   [s(psi) * c(th), c(psi) * c(phi) + s(phi) * s(th) * s(psi), -c(psi) * s(phi) + s(th) * s(psi) * c(phi)],
                   [-s(th), c(th) * s(phi), c(th) * c(phi)]])
    Tm = np.array([[1, s(psi) * s(th) / c(th), c(phi) * s(th) / c(th)], [0, c(phi), s(phi)], [0, s(phi) / c(th), c(phi) / c(th)]])
    wf = np.concatenate([Rz @ xn[12:15], Tm @ xn[15:18]])
    mp = np.array([xn[12] / p["compensate_coef"], xn[13] / p["compensate_coef"], xn[14] / p["rotor_constant"], xn[17] / p["rotor_constant"]])
    return wf, mp


class Doubles:
    """the two double-precision implementations whose own error against the reference sets the bar: the C oracle (oracle/
    bluerov2_ekf_oracle.c, pivoted LU) and the numpy restatement test_oracle_ekf.np_update, both with the parameters `par_vec`"""

    def __init__(self, par_vec):
        import test_oracle_ekf as T
        from oracle.oracle_ffi import EkfOracle
        self.T, self.ekf, self.p = T, EkfOracle(), par_dict(par_vec)
        par_apply(self.ekf.par, par_vec)
        self.ekf.lib.orc_ekf_derive(self.ekf.par)
        self.c = T.np_consts(self.ekf.par)

    def _prediction(self, rk4, jac, x, P, thrust, y12):
        tau = self.c["K"] @ thrust
        xp, F = rk4(x, tau), jac(x, tau)
        return (xp, F @ P @ F.T + np.diag(self.c["Q"])) + np_outputs(self.p, xp, y12)

    def oracle(self, x, P, thrust, y12, acc, prediction=False):
        """(x, P, wf, mpc_p) of one tick; prediction=True: of the prediction alone, from the oracle's own RK4 map and Jacobian"""
        if prediction:
            return self._prediction(self.ekf.rk4, self.ekf.jac_F, x, P, thrust, y12)
        xo, Po = np.array(x, dtype=np.float64)[None].copy(), np.array(P, dtype=np.float64)[None].copy()
        wf, mp, rc = self.ekf.update(xo, Po, thrust[None], y12[None], acc[None])
        assert rc == 0
        return xo[0], Po[0], wf[0], mp[0]

    def numpy(self, x, P, thrust, y12, acc, prediction=False, update=None):
        """the same of the numpy restatement (update: a variant of np_update with the same signature)"""
        T, c = self.T, self.c
        if prediction:
            return self._prediction(lambda z, tau: T.np_rk4(c, z, tau), lambda z, tau: T.np_fd(lambda w: T.np_rk4(c, w, tau), z, c["fd_step"]),
                                    x, P, thrust, y12)
        xn, Pn = (update or T.np_update)(c, x, P, thrust, y12, acc)
        return (xn, Pn) + np_outputs(self.p, xn, y12)

    def consistent_inputs(self, rng, x):
        """thrust, y12, acc of one filter with an innovation of realistic size, as tests/test_gpu_ekf.py draws them"""
        T, c = self.T, self.c
        thrust = rng.uniform(-4, 4, 6)
        tau = c["K"] @ thrust
        acc = T.np_f(c, x, tau)[6:12] + rng.normal(size=6) * 0.01
        y12 = T.np_rk4(c, x, tau)[:12] + rng.normal(size=12) * 1e-3
        return thrust, y12, acc


def _h21col(k):
    return k in (3, 4) or 6 <= k < 12


def fd_rounding_bound(D, x, P, thrust, y12, acc):
    """First-order bound of what the ROUNDING of the two forward differences does to a tick's x, P, wf, mpc_p, scaled like the errors [4].
    In plain numpy (a bound needs no digits), from the restatement's own F, H, S.

    An entry of F is (f1_j - f0_j) / d.  Each of the two values of the RK4 map carries the roundings of its four stage sums, half an ulp of the
    state each (as tests/test_gpu_model_exact._rounding_bound counts them), and those of the increments: a term of a model row is a product of
    up to four factors, a sine or cosine good to 1.5 ulp among them, summed with up to seven others -- 8 x 2^-53 of the sum A_j of the terms'
    absolute values, times dt.  So delta_j = 2^-53 (4 max(|x_j|, |x_pred_j|) + 8 dt A_j) and |dF_ji| <= 2 delta_j / d wherever the entry is not
    an exact zero of the pattern; rows 12..17 pass their state through: ((x_j + d) - x_j) / d, one rounding of x_j + d.  The same for H with
    the terms of h (sum of absolute values B_j, no stage sums), rows 0..11 passing x_pred through.  dF and dH are carried to first order,
    entry by entry with absolute values, through P_pred = F P F' + Q, S, the gain, x_new and the Joseph form (S^-1 as numpy gives it); the
    values' own roundings reach x_new through |I - K H| delta and |K| delta_h.  What elimination and the products round is NOT in it."""
    T, c, p = D.T, D.c, D.p
    u, d, dt, n = 2.0 ** -53, c["fd_step"], c["dt"], N
    tau = c["K"] @ thrust
    y = np.concatenate([y12, tau])
    rk4 = lambda z: T.np_rk4(c, z, tau)      # noqa: E731
    h = lambda z: T.np_h(c, z, acc)          # noqa: E731
    F, xp = T.np_fd(rk4, x, d), rk4(x)
    H, yp = T.np_fd(h, xp, d), h(xp)

    def terms(z, a=None):
        """the sums of the absolute values of the terms of the model's rows 0..11 at z (a: of h's rows 12..17 instead, with M a for tau)"""
        phi, th, psi = z[3:6]
        vu, vv, vw, wp, wq, wr = z[6:12]
        m, bo, mzg = c["mass"], c["bouyancy"], c["mass"] * c["ZG"] * c["g"]
        sph, cph, sth, cth = abs(np.sin(phi)), abs(np.cos(phi)), abs(np.sin(th)), abs(np.cos(th))
        damp = np.abs(c["Dl"] * z[6:12]) + np.abs(c["Dnl"] * z[6:12] * z[6:12])
        body = np.array([m * abs(wr * vv) + m * abs(wq * vw) + bo * sth, m * abs(wr * vu) + m * abs(wp * vw) + bo * cth * sph,
                         m * abs(wq * vu) + m * abs(wp * vv) + bo * cth * cph, abs((c["Iy"] - c["Iz"]) * wq * wr) + mzg * cth * sph,
                         abs((c["Iz"] - c["Ix"]) * wp * wr) + mzg * sth, abs((c["Iy"] - c["Ix"]) * wp * wq)])
        if a is not None:
            return np.abs(np.diag(c["M"]) * a) + body + np.abs(z[12:18]) + damp
        kin = np.concatenate([np.full(3, np.abs(z[6:9]).sum()), np.full(3, np.abs(z[9:12]).sum() / cth)])      # |R| <= 1, |T| <= 1 / cos(theta)
        return np.concatenate([kin, np.diag(c["invM"]) * (np.abs(tau) + body + np.abs(z[12:18]) + damp)])

    delta_f = np.zeros(n); delta_h = np.zeros(n)
    delta_f[:12] = u * (4 * np.maximum(np.abs(x[:12]), np.abs(xp[:12])) + 8 * dt * terms(x))
    delta_h[12:] = u * 8 * terms(xp, acc)
    eF, eH = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if (j == i) if i < 3 else (j < 12 or j == i):
                eF[j, i] = 2 * delta_f[j] / d if j < 12 else u * (abs(x[j]) + d) / d
            if j == i or (j >= 12 and _h21col(i)):
                eH[j, i] = 2 * delta_h[j] / d if j >= 12 else u * (abs(xp[j]) + d) / d
    Pp = F @ P @ F.T + np.diag(c["Q"])
    Si = np.linalg.inv(H @ Pp @ H.T + np.eye(n) * c["R"])
    K = Pp @ H.T @ Si
    J = np.eye(n) - K @ H
    ye = y - yp
    xn, Pn = xp + K @ ye, J @ Pp @ J.T + c["R"] * K @ K.T
    bx = np.abs(J) @ delta_f + np.abs(K) @ delta_h
    bP = np.zeros((n, n))
    FP, R = F @ P, c["R"]
    for j, i in zip(*np.nonzero(eF)):
        dPp = np.zeros((n, n)); dPp[j, :] = FP[:, i]; dPp = dPp + dPp.T      # dF P F' + F P dF', dF = e_j e_i'
        dK = (dPp @ H.T - K @ (H @ dPp @ H.T)) @ Si
        dJ = -dK @ H
        t1, t2 = dJ @ Pp @ J.T, R * dK @ K.T
        bx += np.abs(dK @ ye) * eF[j, i]
        bP += np.abs(t1 + t1.T + J @ dPp @ J.T + t2 + t2.T) * eF[j, i]
    PpHt = Pp @ H.T
    for j, i in zip(*np.nonzero(eH)):
        dH = np.zeros((n, n)); dH[j, i] = 1.0
        t0 = dH @ PpHt
        dK = (Pp @ dH.T - K @ (t0 + t0.T)) @ Si
        dJ = -dK @ H - K @ dH
        t1, t2 = dJ @ Pp @ J.T, R * dK @ K.T
        bx += np.abs(dK @ ye) * eH[j, i]
        bP += np.abs(t1 + t1.T + t2 + t2.T) * eH[j, i]
    phi, th, psi = y12[3:6]
    cth = abs(np.cos(th))
    bwf = np.concatenate([np.full(3, bx[12:15].sum()), np.full(3, bx[15:18].sum() / cth)])
    wf, mp = np_outputs(p, xn, y12)
    bmp = bx[[12, 13, 14, 17]] / np.array([p["compensate_coef"], p["compensate_coef"], p["rotor_constant"], p["rotor_constant"]])
    return np.array([(bx / np.maximum(1.0, np.abs(xn))).max(), bP.max() / np.abs(Pn).max(), (bwf / np.maximum(1.0, np.abs(wf))).max(),
                     (bmp / np.maximum(1.0, np.abs(mp))).max()])


def errors(got, ref):
    """scaled errors of (x, P, wf, mpc_p) against the reference's, in the order of QUANTITIES"""
    return np.array([err_x(got[0], ref[0]), err_P(got[1], ref[1]), err_x(got[2], ref[2]), err_x(got[3], ref[3])])


QUANTITIES = ("x", "P", "wf", "mpc_p")


class ExactEkf:
    def __init__(self, par_vec, digits=DIGITS):
        import mpmath
        self.mp = mp = mpmath.mp.clone()
        mp.dps = int(digits)
        self.sin, self.cos = mp.sin, mp.cos
        p = par_dict(par_vec)
        n = self.num
        for f in ("dt", "mass", "Ix", "Iy", "Iz", "ZG", "g", "bouyancy", "R", "fd_step", "compensate_coef", "rotor_constant"):
            setattr(self, f, n(p[f]))
        self.Dl, self.Dnl, self.Q = [n(v) for v in p["Dl"]], [n(v) for v in p["Dnl"]], [n(v) for v in p["Q"]]
        self.K = [[n(p["K"][i * 6 + j]) for j in range(6)] for i in range(6)]
        am = [n(v) for v in p["added_mass"]]
        M = mp.zeros(6, 6)
        for i, v in enumerate((self.mass + am[0], self.mass + am[1], self.mass + am[2], self.Ix + am[3], self.Iy + am[4], self.Iz + am[5])):
            M[i, i] = v
        M[0, 4] = self.mass * self.ZG; M[1, 3] = -self.mass * self.ZG; M[3, 1] = -self.mass * self.ZG; M[4, 0] = self.mass * self.ZG
        Mi = mp.inverse(M)
        self.Md, self.iMd = [M[i, i] for i in range(6)], [Mi[i, i] for i in range(6)]
        self.zero, self.one = mp.mpf(0), mp.mpf(1)

    def num(self, v):
        return v if isinstance(v, self.mp.mpf) else self.mp.mpf(float(v))

    def vec(self, a, n):
        a = list(np.asarray(a).ravel()) if isinstance(a, np.ndarray) else list(a)
        assert len(a) == n, (len(a), n)
        return [self.num(v) for v in a]

    def mat(self, A):
        assert len(A) == N and all(len(row) == N for row in A)
        return [[self.num(v) for v in row] for row in A]

    # ---- the model ----------------------------------------------------------------------------------------------------------------------------
    def _rot(self, phi, th, psi):
        s, c = self.sin, self.cos
        sph, cph, sth, cth, sps, cps = s(phi), c(phi), s(th), c(th), s(psi), c(psi)
        Rib = [[cps * cth, -sps * cph + cps * sth * sph, sps * sph + cps * cph * sth],
               [sps * cth, cps * cph + sph * sth * sps, -cps * sph + sth * sps * cph],
               [-sth, cth * sph, cth * cph]]
        Tm = [[self.one, sps * sth / cth, cph * sth / cth], [self.zero, cph, sph], [self.zero, sph / cth, cph / cth]]
        return Rib, Tm

    def _terms(self, x):
        """damping [6] and the Coriolis / restoring terms of the six dynamic rows as they stand in f (h has them negated)"""
        phi, th = x[3], x[4]
        u, v, w, p, q, r = x[6:12]
        m, bo, mzg = self.mass, self.bouyancy, self.mass * self.ZG * self.g
        s, c = self.sin, self.cos
        damp = [self.Dl[i] * x[6 + i] + self.Dnl[i] * abs(x[6 + i]) * x[6 + i] for i in range(6)]
        body = [m * r * v - m * q * w - bo * s(th),
                -m * r * u + m * p * w + bo * c(th) * s(phi),
                m * q * u - m * p * v + bo * c(th) * c(phi),
                (self.Iy - self.Iz) * q * r - mzg * c(th) * s(phi),
                (self.Iz - self.Ix) * p * r - mzg * s(th),
                -(self.Iy - self.Ix) * p * q]
        return damp, body

    def f(self, x, tau):
        Rib, Tm = self._rot(x[3], x[4], x[5])
        damp, body = self._terms(x)
        o = [sum((Rib[i][j] * x[6 + j] for j in range(3)), self.zero) for i in range(3)]
        o += [sum((Tm[i][j] * x[9 + j] for j in range(3)), self.zero) for i in range(3)]
        o += [self.iMd[i] * (tau[i] + body[i] + x[12 + i] + damp[i]) for i in range(6)]
        return o + [self.zero] * 6

    def rk4(self, x, tau):
        dt = self.dt
        k1 = [v * dt for v in self.f(x, tau)]
        k2 = [v * dt for v in self.f([a + b / 2 for a, b in zip(x, k1)], tau)]
        k3 = [v * dt for v in self.f([a + b / 3 for a, b in zip(x, k2)], tau)]      # the third stage at x + k2 / 3, as the filter has it
        k4 = [v * dt for v in self.f([a + b for a, b in zip(x, k3)], tau)]
        return [a + (b + 2 * c + 2 * d + e) / 6 for a, b, c, d, e in zip(x, k1, k2, k3, k4)]

    def h(self, x, acc):
        damp, body = self._terms(x)
        return list(x[:12]) + [self.Md[i] * acc[i] - body[i] - x[12 + i] - damp[i] for i in range(6)]

    def fd(self, fun, x):
        """forward differences with the filter's step: J[j][i] = (fun(x + d e_i)[j] - fun(x)[j]) / d"""
        d = self.fd_step
        f0 = fun(x)
        J = [[None] * N for _ in range(N)]
        for i in range(N):
            x1 = list(x); x1[i] = x1[i] + d
            f1 = fun(x1)
            for j in range(N):
                J[j][i] = (f1[j] - f0[j]) / d
        return f0, J

    # ---- linear algebra on lists -----------------------------------------------------------------------------------------------------------------
    def mm(self, A, B):
        Bt = list(zip(*B))
        return [[sum((a * b for a, b in zip(row, col)), self.zero) for col in Bt] for row in A]

    @staticmethod
    def tr(A):
        return [list(r) for r in zip(*A)]

    def eliminate(self, S):
        """Gauss-Jordan on [S | I] WITHOUT row exchanges: (the pivots met, up to and including the first that is not positive; S^-1 or None)"""
        a = [list(S[i]) + [self.one if i == j else self.zero for j in range(N)] for i in range(N)]
        piv = []
        for k in range(N):
            p = a[k][k]
            piv.append(p)
            if not p > 0:
                return piv, None
            a[k] = [v / p for v in a[k]]
            for i in range(N):
                if i != k:
                    fct = a[i][k]
                    a[i] = [vi - fct * vk for vi, vk in zip(a[i], a[k])]
        return piv, [row[N:] for row in a]

    # ---- one tick ------------------------------------------------------------------------------------------------------------------------------------
    def tick(self, x, P, thrust, y12, acc):
        """x [18], P [18][18] (doubles, or mpf carried from the tick before); thrust [6], y12 [12], acc [6] doubles.  Everything returned is mpf."""
        x, P = self.vec(x, N), self.mat(P)
        thrust, y12, acc = self.vec(thrust, 6), self.vec(y12, 12), self.vec(acc, 6)
        tau = [sum((self.K[i][j] * thrust[j] for j in range(6)), self.zero) for i in range(6)]
        y = y12 + tau
        xp, F = self.fd(lambda z: self.rk4(z, tau), x)
        Pp = self.mm(self.mm(F, P), self.tr(F))
        for i in range(N):
            Pp[i][i] += self.Q[i]
        yp, H = self.fd(lambda z: self.h(z, acc), xp)
        PHt = self.mm(Pp, self.tr(H))
        S = self.mm(H, PHt)
        for i in range(N):
            S[i][i] += self.R
        piv, Si = self.eliminate(S)
        if Si is None:
            xn, Pn, status = list(xp), [list(r) for r in Pp], 1
        else:
            Kal = self.mm(PHt, Si)
            ye = [a - b for a, b in zip(y, yp)]
            xn = [a + sum((k * e for k, e in zip(row, ye)), self.zero) for a, row in zip(xp, Kal)]
            KH = self.mm(Kal, H)
            J = [[(self.one if i == j else self.zero) - KH[i][j] for j in range(N)] for i in range(N)]
            JPJ = self.mm(self.mm(J, Pp), self.tr(J))
            KK = self.mm(Kal, self.tr(Kal))
            Pn = [[JPJ[i][j] + self.R * KK[i][j] for j in range(N)] for i in range(N)]
            status = 0
        Rib, Tm = self._rot(y12[3], y12[4], y12[5])
        wf = [sum((Rib[i][j] * xn[12 + j] for j in range(3)), self.zero) for i in range(3)]
        wf += [sum((Tm[i][j] * xn[15 + j] for j in range(3)), self.zero) for i in range(3)]
        mp = [xn[12] / self.compensate_coef, xn[13] / self.compensate_coef, xn[14] / self.rotor_constant, xn[17] / self.rotor_constant]
        return dict(x_pred=xp, P_pred=Pp, pivots=piv, x_new=xn, P_new=Pn, wf=wf, mpc_p=mp, status=status)

    def rounded(self, out):
        """a tick's result rounded to double (mpmath rounds to nearest); the pivots not met are NaN"""
        f = float
        piv = np.full(N, np.nan)
        piv[:len(out["pivots"])] = [f(v) for v in out["pivots"]]
        return dict(x_pred=np.array([f(v) for v in out["x_pred"]]), P_pred=np.array([[f(v) for v in r] for r in out["P_pred"]]), pivots=piv,
                    x_new=np.array([f(v) for v in out["x_new"]]), P_new=np.array([[f(v) for v in r] for r in out["P_new"]]),
                    wf=np.array([f(v) for v in out["wf"]]), mpc_p=np.array([f(v) for v in out["mpc_p"]]), status=out["status"])

    def tick_double(self, x, P, thrust, y12, acc):
        return self.rounded(self.tick(x, P, thrust, y12, acc))
