"""One tick of the error-state Kalman filter with IMU disturbance observer (include/bluerov2_nmpc_eskf.h, brov_eskf_*) in far more than double
precision, and the same formulas in plain numpy: the yardstick of tests/test_eskf_exact_cpu.py, tests/test_gpu_eskf_exact.py and
tests/test_gpu_eskf_loop.py (fixture tests/golden/eskf_exact.npz, scripts/make_eskf_exact_golden.py).  Written from the formulas of the header,
not from the kernel.

Nominal state x [22] = [p_I(3) | v_I(3) | q(4: w, x, y, z) | b_g(3) | b_a(3) | g_I(3) | xi(3)]; covariance P [21][21] over the error state
[dp, dv, dtheta, db_g, db_a, dg, dxi].  A tick:

    q, q_meas <- q / |q|, q_meas / |q_meas|                                 (every quaternion product is followed by the same normalisation)
  predict, IMU sample (a_m, w_m):  a = a_m - b_a, w = w_m - b_g, R = R(q)
    p += v dt + (R a) dt^2 / 2 + g_I dt^2 / 2;   v += (R a) dt + g_I dt      (old R, and p takes the old v);   q = q * exp(w dt)
    F = I but  F[3:6,6:9] = -R hat(a) dt,  F[3:6,12:15] = -R dt  (the NEW R),  F[6:9,6:9] = exp(-w dt),  F[0:3,3:6] = F[3:6,15:18] = I dt,
    F[6:9,9:12] = -I dt;   P = F P F' + diag(Q)
  update:  y = [p_gps - p | v_gps - v | log(q^-1 * q_meas) | tau3 - (Mrb3 - xi + Ma3 + D3 + g3)]
    Mrb3 = [m a0 + m ZG w1, m a1 - m ZG w0, m a2];   Ma3_i = added_mass[i] (a_i + gB_i), gB = R(q_meas)' (0, 0, -g);
    D3_i = (-Dl[i] - Dnl[i] |vB_i|) vB_i, vB = R(q)' v;   g3 = (m g - bouyancy) [sin th, -cos th sin ph, -cos th cos ph], roll ph and pitch th of q;
    tau3 = the first three rows of K thrust
    H = 0 but H[0:3,0:3] = H[3:6,3:6] = H[6:9,6:9] = I, H[9:12,18:21] = -I;   S = H P H' + diag(R12), eliminated WITHOUT row exchanges;
    a pivot that is not positive: status 1, state and covariance stay at the prediction.  Else Kal = P H' S^-1, dx = Kal y, P = (I - Kal H) P,
    p += dx[0:3], v += vel_inject dx[3:6], q = q * exp(dx[6:9]), xi += dx[18:21], and with inject_bias_g: b_g, b_a, g_I += dx[9:12], [12:15], [15:18]
  outputs: xi, xi_world = R(q) xi, mpc_p = [xi0 / compensate_coef, xi1 / compensate_coef, xi2 / rotor_constant, 0]

    exp(phi) = [cos(|phi| / 2), sin(|phi| / 2) phi / |phi|];   log(q) = 2 atan(|v| / w) v / |v|  (atan, not atan2: q and -q have the same logarithm)

Every input is taken as the exact value of the double it is given as, the parameters too."""
import numpy as np

NX, NE, NY = 22, 21, 12
DIGITS = 60
PAR_FIELDS = (("dt", 1), ("gps_dt", 1), ("mass", 1), ("ZG", 1), ("g", 1), ("bouyancy", 1), ("added_mass", 6), ("Dl", 6), ("Dnl", 6), ("K", 36),
              ("Q", 21), ("R12", 12), ("vel_inject", 1), ("compensate_coef", 1), ("rotor_constant", 1), ("inject_bias_g", 1))
NPAR = sum(n for _, n in PAR_FIELDS)
IU = np.triu_indices(NE)
HSEL = (0, 1, 2, 3, 4, 5, 6, 7, 8, 18, 19, 20)      # H's row a selects error state HSEL[a] ...
HSGN = (1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1)      # ... with this sign
QUANTITIES = ("x", "P", "xi_world", "mpc_p")


def par_vector(par):
    """the fields of a brov_eskf_params (bluerov2_amd.EskfParams) as one vector"""
    return np.concatenate([np.atleast_1d(np.array(getattr(par, f), dtype=np.float64)) for f, _ in PAR_FIELDS])


def par_apply(par, vec):
    vec = np.asarray(vec, dtype=np.float64)
    assert vec.shape == (NPAR,)
    o = 0
    for f, n in PAR_FIELDS:
        if f == "inject_bias_g":
            setattr(par, f, int(vec[o]))
        elif n == 1:
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


def default_par_vector():
    """the defaults of brov_eskf_default_params, as plain numbers (ImuDo.h:101-110, Config.cpp:175-180, launch/config/imudo.yaml, Eskf.cpp:103,184;
    compensate_coef and rotor_constant those of brov_ekf_params) -- tests/test_eskf_abi.py holds the library's defaults to this vector"""
    K = [0.7071067811847433, 0.7071067811847433, -0.7071067811919605, -0.7071067811919605, 0.0, 0.0,
         0.7071067811883519, -0.7071067811883519, 0.7071067811811348, -0.7071067811811348, 0.0, 0.0,
         0, 0, 0, 0, 1, 1,
         0.051265241636155506, -0.05126524163615552, 0.05126524163563227, -0.05126524163563227, -0.11050000000000001, 0.11050000000000003,
         -0.05126524163589389, -0.051265241635893896, 0.05126524163641713, 0.05126524163641713, -0.002499999999974481, -0.002499999999974481,
         0.16652364696949604, -0.16652364696949604, -0.17500892834341342, 0.17500892834341342, 0.0, 0.0]
    return np.array([1.0 / 50.0, 1.0 / 30.0, 11.26, 0.02, 9.81, 0.661618] + [1.7182, 0, 5.468, 0, 1.2481, 0.4006] + [-11.7391, -20, -31.8678, -25, -44.9085, -5]
                    + [-18.18, -21.66, -36.99, -1.55, -1.55, -1.55] + K + [0.001] * 21 + [0.01] * 3 + [0.02] * 3 + [0.0006] * 3 + [0.012] * 3
                    + [2.0, 0.032546960744430276, 0.026546960744430276, 0.0], dtype=np.float64)


def to_triu(P):
    return np.asarray(P)[..., IU[0], IU[1]]


def from_triu(v):
    v = np.asarray(v)
    P = np.zeros(v.shape[:-1] + (NE, NE))
    P[..., IU[0], IU[1]] = v
    P[..., IU[1], IU[0]] = v
    return P


def err_x(got, ref):
    """|got - ref| / max(1, |ref|), the worst entry of each filter (NaN where got is NaN); also for xi_world and mpc_p"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max(axis=-1)


def err_state(got, ref):
    """err_x of a nominal state [.., 22], its quaternion compared up to sign: min(|q - q_ref|, |q + q_ref|)"""
    got, ref = np.array(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    flip = np.abs(got[..., 6:10] + ref[..., 6:10]).max(axis=-1) < np.abs(got[..., 6:10] - ref[..., 6:10]).max(axis=-1)
    got[..., 6:10] = np.where(flip[..., None], -got[..., 6:10], got[..., 6:10])
    return err_x(got, ref)


def err_P(got, ref):
    """|got - ref| / max |ref| per filter, the worst entry of each"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return (np.abs(got - ref).max(axis=(-2, -1))) / np.abs(ref).max(axis=(-2, -1))


def errors(got, ref):
    """scaled errors of (x, P, xi_world, mpc_p) against the reference's, in the order of QUANTITIES"""
    return np.array([err_state(got[0], ref[0]), err_P(got[1], ref[1]), err_x(got[2], ref[2]), err_x(got[3], ref[3])])


# ======================================================================================================================================================
# the numpy restatement (double)
# ======================================================================================================================================================
def np_hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def np_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def np_qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def np_unit(q):
    return q / np.sqrt(q @ q)


def np_exp(phi):
    t2 = phi @ phi
    t = np.sqrt(t2)
    if t2 < 2.0 ** -40:      # the series: sin(t / 2) / t = 1/2 - t^2 / 48 + ..., cos(t / 2) = 1 - t^2 / 8 + ...
        return np.concatenate([[1.0 - t2 / 8.0], (0.5 - t2 / 48.0) * phi])
    return np.concatenate([[np.cos(t / 2)], (np.sin(t / 2) / t) * phi])


def np_log(q):
    w, v = q[0], q[1:]
    n2 = v @ v
    n = np.sqrt(n2)
    if n2 < 2.0 ** -40:      # 2 atan(n / w) / n = 2 / w - 2 n^2 / (3 w^3) + ...
        return (2.0 / w - 2.0 * n2 / (3.0 * w * w * w)) * v
    if w == 0.0:
        return (np.pi / n) * v
    return (2.0 * np.arctan(n / w) / n) * v


def np_F(p, R_new, a, w):
    """the dense 21 x 21 F"""
    dt = p["dt"]
    F = np.eye(NE)
    F[0:3, 3:6] = np.eye(3) * dt
    F[3:6, 6:9] = -R_new @ np_hat(a) * dt
    F[3:6, 12:15] = -R_new * dt
    F[3:6, 15:18] = np.eye(3) * dt
    F[6:9, 6:9] = np_rot(np_exp(-w * dt))
    F[6:9, 9:12] = -np.eye(3) * dt
    return F


def np_H():
    H = np.zeros((NY, NE))
    for a in range(NY):
        H[a, HSEL[a]] = HSGN[a]
    return H


def np_predict_cov(p, P, R_new, a, w, structured=True):
    """F P F' + diag(Q): dense, or from the structure -- F = I + six 3 x 3 blocks, so B = P F' changes columns 0..8 and F B rows 0..8"""
    if not structured:
        F = np_F(p, R_new, a, w)
        return F @ P @ F.T + np.diag(p["Q"])
    dt = p["dt"]
    M1, M2, E = -R_new @ np_hat(a) * dt, -R_new * dt, np_rot(np_exp(-w * dt))
    B = P.copy()
    B[:, 0:3] = P[:, 0:3] + dt * P[:, 3:6]
    B[:, 3:6] = P[:, 3:6] + P[:, 6:9] @ M1.T + P[:, 12:15] @ M2.T + dt * P[:, 15:18]
    B[:, 6:9] = P[:, 6:9] @ E.T - dt * P[:, 9:12]
    Pn = B.copy()
    Pn[0:3] = B[0:3] + dt * B[3:6]
    Pn[3:6] = B[3:6] + M1 @ B[6:9] + M2 @ B[12:15] + dt * B[15:18]
    Pn[6:9] = E @ B[6:9] - dt * B[9:12]
    return Pn + np.diag(p["Q"])


def np_S(p, P, structured=True):
    """(S, P H'): dense, or as a signed gather from P plus the diagonal, and twelve signed columns of P"""
    if not structured:
        H = np_H()
        return H @ P @ H.T + np.diag(p["R12"]), P @ H.T
    sel, sgn = np.array(HSEL), np.array(HSGN, dtype=np.float64)
    return P[np.ix_(sel, sel)] * np.outer(sgn, sgn) + np.diag(p["R12"]), P[:, sel] * sgn


def np_eliminate(S):
    """Gauss-Jordan on [S | I] without row exchanges: (pivots met up to and including the first that is not positive, S^-1 or None)"""
    n = len(S)
    a = np.hstack([np.array(S, dtype=np.float64), np.eye(n)])
    piv = []
    for k in range(n):
        pk = a[k, k]
        piv.append(pk)
        if not pk > 0:
            return piv, None
        a[k] = a[k] / pk
        for i in range(n):
            if i != k:
                a[i] = a[i] - a[i, k] * a[k]
    return piv, a[:, n:]


def np_innovation(p, x, imu, gps_p, gps_v, qm, thrust):
    pos, v, q, bg, ba, xi = x[0:3], x[3:6], x[6:10], x[10:13], x[13:16], x[19:22]
    a, w = imu[0:3] - ba, imu[3:6] - bg
    m, zg = p["mass"], p["ZG"]
    R = np_rot(q)
    vB = R.T @ v
    gB = np_rot(qm).T @ np.array([0.0, 0.0, -p["g"]])
    mrb = np.array([m * a[0] + m * zg * w[1], m * a[1] - m * zg * w[0], m * a[2]])
    ma = p["added_mass"][:3] * (a + gB)
    d3 = (-p["Dl"][:3] - p["Dnl"][:3] * np.abs(vB)) * vB
    ph = np.arctan2(2 * (q[0] * q[1] + q[2] * q[3]), 1 - 2 * (q[1] * q[1] + q[2] * q[2]))
    th = np.arcsin(2 * (q[0] * q[2] - q[3] * q[1]))
    g3 = (m * p["g"] - p["bouyancy"]) * np.array([np.sin(th), -np.cos(th) * np.sin(ph), -np.cos(th) * np.cos(ph)])
    tau3 = p["K"].reshape(6, 6)[:3] @ thrust
    qc = np.array([q[0], -q[1], -q[2], -q[3]])
    return np.concatenate([gps_p - pos, gps_v - v, np_log(np_unit(np_qmul(qc, qm))), tau3 - (mrb - xi + ma + d3 + g3)])


def np_outputs(p, x):
    xi = x[19:22]
    return xi.copy(), np_rot(x[6:10]) @ xi, np.array([xi[0] / p["compensate_coef"], xi[1] / p["compensate_coef"], xi[2] / p["rotor_constant"], 0.0])


def np_tick(p, x, P, imu, gps_p=None, gps_v=None, q_meas=None, thrust=None, update=True, structured=True):
    """one tick in double; p = par_dict(vector).  Returns a dict like ExactEskf.tick_double"""
    x, P, imu = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64), np.asarray(imu, dtype=np.float64)
    dt = p["dt"]
    x[6:10] = np_unit(x[6:10])
    a, w = imu[0:3] - x[13:16], imu[3:6] - x[10:13]
    Ra = np_rot(x[6:10]) @ a
    g = x[16:19]
    xp = x.copy()
    xp[0:3] = x[0:3] + x[3:6] * dt + 0.5 * Ra * dt * dt + 0.5 * g * dt * dt
    xp[3:6] = x[3:6] + Ra * dt + g * dt
    xp[6:10] = np_unit(np_qmul(x[6:10], np_exp(w * dt)))
    Pp = np_predict_cov(p, P, np_rot(xp[6:10]), a, w, structured)
    out = dict(x_pred=xp, P_pred=Pp, pivots=np.full(NY, np.nan), status=0)
    xn, Pn = xp, Pp
    if update:
        qm = np_unit(np.asarray(q_meas, dtype=np.float64))
        y = np_innovation(p, xp, imu, np.asarray(gps_p, dtype=np.float64), np.asarray(gps_v, dtype=np.float64), qm, np.asarray(thrust, dtype=np.float64))
        S, PHt = np_S(p, Pp, structured)
        piv, Si = np_eliminate(S)
        out["pivots"][:len(piv)] = piv
        out["y"] = y
        if Si is None:
            out["status"] = 1
        else:
            Kal = PHt @ Si
            dx = Kal @ y
            Pn = Pp - Kal @ PHt.T if structured else (np.eye(NE) - Kal @ np_H()) @ Pp
            xn = xp.copy()
            xn[0:3] += dx[0:3]
            xn[3:6] += p["vel_inject"] * dx[3:6]
            xn[6:10] = np_unit(np_qmul(xp[6:10], np_exp(dx[6:9])))
            xn[19:22] += dx[18:21]
            if p["inject_bias_g"]:
                xn[10:19] += dx[9:18]
    xi, xw, mp = np_outputs(p, xn)
    out.update(x_new=xn, P_new=Pn, xi=xi, xi_world=xw, mpc_p=mp)
    return out


def np_rot_euler(ph, th, ps):
    s, c = np.sin, np.cos
    return np.array([[c(ps) * c(th), -s(ps) * c(ph) + c(ps) * s(th) * s(ph), s(ps) * s(ph) + c(ps) * c(ph) * s(th)],
                     [s(ps) * c(th), c(ps) * c(ph) + s(ph) * s(th) * s(ps), -c(ps) * s(ph) + s(th) * s(ps) * c(ph)],
                     [-s(th), c(th) * s(ph), c(th) * c(ph)]])


def np_inputs_from_state(p, xs, thrust, v_prev=None, p_prev=None):
    """what brov_eskf_update_from_solver synthesises from a 12-state xs = (x, y, z, phi, theta, psi, u, v, w, p, q, r) and the applied thrusts:
    (imu [6], gps_p, gps_v, q_meas, thrust, v_I); prev = None: the first call after a reset, the previous values equal the current ones"""
    xs = np.asarray(xs, dtype=np.float64)
    ph, th, ps = xs[3:6]
    R = np_rot_euler(ph, th, ps)
    vI = R @ xs[6:9]
    vp = vI if v_prev is None else np.asarray(v_prev)
    pp = xs[0:3] if p_prev is None else np.asarray(p_prev)
    gI = np.array([0.0, 0.0, -p["g"]])
    am = R.T @ ((vI - vp) / p["dt"] - gI)
    c, s = np.cos, np.sin
    qm = np.array([c(ps / 2) * c(th / 2) * c(ph / 2) + s(ps / 2) * s(th / 2) * s(ph / 2), c(ps / 2) * c(th / 2) * s(ph / 2) - s(ps / 2) * s(th / 2) * c(ph / 2),
                   c(ps / 2) * s(th / 2) * c(ph / 2) + s(ps / 2) * c(th / 2) * s(ph / 2), s(ps / 2) * c(th / 2) * c(ph / 2) - c(ps / 2) * s(th / 2) * s(ph / 2)])
    return np.concatenate([am, xs[9:12]]), xs[0:3].copy(), (xs[0:3] - pp) / p["gps_dt"], qm, np.asarray(thrust, dtype=np.float64), vI


# ======================================================================================================================================================
# the same at 60 digits
# ======================================================================================================================================================
class ExactEskf:
    def __init__(self, par_vec, digits=DIGITS):
        import mpmath
        self.mp = mp = mpmath.mp.clone()
        mp.dps = int(digits)
        p = par_dict(par_vec)
        n = self.num
        for f in ("dt", "gps_dt", "mass", "ZG", "g", "bouyancy", "vel_inject", "compensate_coef", "rotor_constant"):
            setattr(self, f, n(p[f]))
        self.inject_bias_g = bool(p["inject_bias_g"])
        self.am, self.Dl, self.Dnl = [n(v) for v in p["added_mass"]], [n(v) for v in p["Dl"]], [n(v) for v in p["Dnl"]]
        self.Q, self.R12 = [n(v) for v in p["Q"]], [n(v) for v in p["R12"]]
        self.K = [[n(p["K"][i * 6 + j]) for j in range(6)] for i in range(6)]
        self.zero, self.one = mp.mpf(0), mp.mpf(1)

    def num(self, v):
        return v if isinstance(v, self.mp.mpf) else self.mp.mpf(float(v))

    def vec(self, a, n):
        a = list(np.asarray(a).ravel()) if isinstance(a, np.ndarray) else list(a)
        assert len(a) == n, (len(a), n)
        return [self.num(v) for v in a]

    def mat(self, A):
        assert len(A) == NE and all(len(row) == NE for row in A)
        return [[self.num(v) for v in row] for row in A]

    # ---- rotations ---------------------------------------------------------------------------------------------------------------------------
    def dot(self, a, b):
        return sum((u * v for u, v in zip(a, b)), self.zero)

    def mv(self, A, v):
        return [self.dot(r, v) for r in A]

    def mm(self, A, B):
        Bt = list(zip(*B))
        return [[self.dot(row, col) for col in Bt] for row in A]

    @staticmethod
    def tr(A):
        return [list(r) for r in zip(*A)]

    def hat(self, v):
        z = self.zero
        return [[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]]

    def rot(self, q):
        w, x, y, z = q
        return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]

    @staticmethod
    def qmul(a, b):
        return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]

    def unit(self, q):
        n = self.mp.sqrt(self.dot(q, q))
        return [v / n for v in q]

    def exp(self, phi):
        t = self.mp.sqrt(self.dot(phi, phi))
        if t == 0:
            return [self.one] + [v / 2 for v in phi]
        s = self.mp.sin(t / 2) / t
        return [self.mp.cos(t / 2)] + [s * v for v in phi]

    def log(self, q):
        w, v = q[0], q[1:]
        n = self.mp.sqrt(self.dot(v, v))
        if n == 0:
            return [self.zero] * 3
        c = self.mp.pi / n if w == 0 else 2 * self.mp.atan(n / w) / n
        return [c * u for u in v]

    def angle(self, phi):
        return self.mp.sqrt(self.dot(phi, phi))

    def rot_euler(self, ph, th, ps):
        s, c = self.mp.sin, self.mp.cos
        return [[c(ps) * c(th), -s(ps) * c(ph) + c(ps) * s(th) * s(ph), s(ps) * s(ph) + c(ps) * c(ph) * s(th)],
                [s(ps) * c(th), c(ps) * c(ph) + s(ph) * s(th) * s(ps), -c(ps) * s(ph) + s(th) * s(ps) * c(ph)],
                [-s(th), c(th) * s(ph), c(th) * c(ph)]]

    # ---- the pieces --------------------------------------------------------------------------------------------------------------------------------
    def F(self, R_new, a, w):
        dt, z, o = self.dt, self.zero, self.one
        F = [[o if i == j else z for j in range(NE)] for i in range(NE)]
        M1 = self.mm(R_new, self.hat(a))
        E = self.rot(self.exp([-v * dt for v in w]))
        for r in range(3):
            F[r][3 + r] = dt
            F[3 + r][15 + r] = dt
            F[6 + r][9 + r] = -dt
            for c in range(3):
                F[3 + r][6 + c] = -M1[r][c] * dt
                F[3 + r][12 + c] = -R_new[r][c] * dt
                F[6 + r][6 + c] = E[r][c]
        return F

    def H(self):
        H = [[self.zero] * NE for _ in range(NY)]
        for a in range(NY):
            H[a][HSEL[a]] = self.one * HSGN[a]
        return H

    def eliminate(self, S):
        """Gauss-Jordan on [S | I] WITHOUT row exchanges: (the pivots met, up to and including the first that is not positive; S^-1 or None)"""
        n = len(S)
        a = [list(S[i]) + [self.one if i == j else self.zero for j in range(n)] for i in range(n)]
        piv = []
        for k in range(n):
            p = a[k][k]
            piv.append(p)
            if not p > 0:
                return piv, None
            a[k] = [v / p for v in a[k]]
            for i in range(n):
                if i != k:
                    fct = a[i][k]
                    a[i] = [vi - fct * vk for vi, vk in zip(a[i], a[k])]
        return piv, [row[n:] for row in a]

    def innovation(self, x, imu, gps_p, gps_v, qm, thrust):
        mp = self.mp
        pos, v, q, bg, ba, xi = x[0:3], x[3:6], x[6:10], x[10:13], x[13:16], x[19:22]
        a = [imu[i] - ba[i] for i in range(3)]
        w = [imu[3 + i] - bg[i] for i in range(3)]
        m, zg = self.mass, self.ZG
        vB = self.mv(self.tr(self.rot(q)), v)
        gB = self.mv(self.tr(self.rot(qm)), [self.zero, self.zero, -self.g])
        mrb = [m * a[0] + m * zg * w[1], m * a[1] - m * zg * w[0], m * a[2]]
        ma = [self.am[i] * (a[i] + gB[i]) for i in range(3)]
        d3 = [(-self.Dl[i] - self.Dnl[i] * abs(vB[i])) * vB[i] for i in range(3)]
        ph = mp.atan2(2 * (q[0] * q[1] + q[2] * q[3]), 1 - 2 * (q[1] * q[1] + q[2] * q[2]))
        th = mp.asin(2 * (q[0] * q[2] - q[3] * q[1]))
        k = m * self.g - self.bouyancy
        g3 = [k * mp.sin(th), -k * mp.cos(th) * mp.sin(ph), -k * mp.cos(th) * mp.cos(ph)]
        tau3 = [self.dot(self.K[i], thrust) for i in range(3)]
        qc = [q[0], -q[1], -q[2], -q[3]]
        att = self.log(self.unit(self.qmul(qc, qm)))
        return ([gps_p[i] - pos[i] for i in range(3)] + [gps_v[i] - v[i] for i in range(3)] + att
                + [tau3[i] - (mrb[i] - xi[i] + ma[i] + d3[i] + g3[i]) for i in range(3)])

    def outputs(self, x):
        xi = x[19:22]
        return list(xi), self.mv(self.rot(x[6:10]), xi), [xi[0] / self.compensate_coef, xi[1] / self.compensate_coef, xi[2] / self.rotor_constant, self.zero]

    # ---- one tick ------------------------------------------------------------------------------------------------------------------------------------
    def tick(self, x, P, imu, gps_p=None, gps_v=None, q_meas=None, thrust=None, update=True):
        """x [22], P [21][21] (doubles, or mpf carried from the tick before); the inputs doubles (or mpf).  Everything returned is mpf."""
        x, P, imu = self.vec(x, NX), self.mat(P), self.vec(imu, 6)
        dt = self.dt
        q = self.unit(x[6:10])
        a = [imu[i] - x[13 + i] for i in range(3)]
        w = [imu[3 + i] - x[10 + i] for i in range(3)]
        Ra = self.mv(self.rot(q), a)
        g = x[16:19]
        xp = list(x)
        for i in range(3):
            xp[i] = x[i] + x[3 + i] * dt + Ra[i] * dt * dt / 2 + g[i] * dt * dt / 2
            xp[3 + i] = x[3 + i] + Ra[i] * dt + g[i] * dt
        xp[6:10] = self.unit(self.qmul(q, self.exp([v * dt for v in w])))
        F = self.F(self.rot(xp[6:10]), a, w)
        Pp = self.mm(self.mm(F, P), self.tr(F))
        for i in range(NE):
            Pp[i][i] += self.Q[i]
        out = dict(x_pred=xp, P_pred=Pp, pivots=[], status=0, angle_pred=self.angle([v * dt for v in w]))
        xn, Pn = xp, Pp
        if update:
            qm = self.unit(self.vec(q_meas, 4))
            y = self.innovation(xp, imu, self.vec(gps_p, 3), self.vec(gps_v, 3), qm, self.vec(thrust, 6))
            H = self.H()
            PHt = self.mm(Pp, self.tr(H))
            S = self.mm(H, PHt)
            for i in range(NY):
                S[i][i] += self.R12[i]
            piv, Si = self.eliminate(S)
            out.update(pivots=piv, y=y, angle_innov=self.angle(y[6:9]))
            if Si is None:
                out["status"] = 1
            else:
                Kal = self.mm(PHt, Si)
                dx = self.mv(Kal, y)
                KH = self.mm(Kal, H)
                J = [[(self.one if i == j else self.zero) - KH[i][j] for j in range(NE)] for i in range(NE)]
                Pn = self.mm(J, Pp)
                xn = list(xp)
                for i in range(3):
                    xn[i] = xp[i] + dx[i]
                    xn[3 + i] = xp[3 + i] + self.vel_inject * dx[3 + i]
                    xn[19 + i] = xp[19 + i] + dx[18 + i]
                xn[6:10] = self.unit(self.qmul(xp[6:10], self.exp(dx[6:9])))
                if self.inject_bias_g:
                    for i in range(9):
                        xn[10 + i] = xp[10 + i] + dx[9 + i]
        xi, xw, mp_ = self.outputs(xn)
        out.update(x_new=xn, P_new=Pn, xi=xi, xi_world=xw, mpc_p=mp_)
        return out

    def rounded(self, out):
        """a tick's result rounded to double (mpmath rounds to nearest); the pivots not met are NaN"""
        f = float
        piv = np.full(NY, np.nan)
        piv[:len(out["pivots"])] = [f(v) for v in out["pivots"]]
        r = dict(pivots=piv, status=out["status"], angle_pred=f(out["angle_pred"]), angle_innov=f(out.get("angle_innov", 0)))
        for k in ("x_pred", "x_new", "xi", "xi_world", "mpc_p"):
            r[k] = np.array([f(v) for v in out[k]])
        for k in ("P_pred", "P_new"):
            r[k] = np.array([[f(v) for v in row] for row in out[k]])
        return r

    def tick_double(self, *a, **kw):
        return self.rounded(self.tick(*a, **kw))

    def inputs_from_state(self, xs, thrust, v_prev=None, p_prev=None):
        """np_inputs_from_state at 60 digits (mpf lists)"""
        mp = self.mp
        xs, thrust = self.vec(xs, 12), self.vec(thrust, 6)
        ph, th, ps = xs[3:6]
        R = self.rot_euler(ph, th, ps)
        vI = self.mv(R, xs[6:9])
        vp = vI if v_prev is None else self.vec(v_prev, 3)
        pp = xs[0:3] if p_prev is None else self.vec(p_prev, 3)
        gI = [self.zero, self.zero, -self.g]
        am = self.mv(self.tr(R), [(vI[i] - vp[i]) / self.dt - gI[i] for i in range(3)])
        c, s = mp.cos, mp.sin
        qm = [c(ps / 2) * c(th / 2) * c(ph / 2) + s(ps / 2) * s(th / 2) * s(ph / 2), c(ps / 2) * c(th / 2) * s(ph / 2) - s(ps / 2) * s(th / 2) * c(ph / 2),
              c(ps / 2) * s(th / 2) * c(ph / 2) + s(ps / 2) * c(th / 2) * s(ph / 2), s(ps / 2) * c(th / 2) * c(ph / 2) - c(ps / 2) * s(th / 2) * s(ph / 2)]
        return am + xs[9:12], xs[0:3], [(xs[i] - pp[i]) / self.gps_dt for i in range(3)], qm, thrust, vI

    def thrust(self, u0):
        """np_thrust at 60 digits"""
        u = self.vec(u0, 4)
        c = self.num(ROTOR)
        return [(-u[0] + u[1] + u[3]) / c, (-u[0] - u[1] - u[3]) / c, (u[0] + u[1] - u[3]) / c, (u[0] - u[1] + u[3]) / c, -u[2] / c, -u[2] / c]


ROTOR = 0.026546960744430276      # the OCP model's rotor constant: the allocation brov_plant_step applies (bluerov2_dob.cpp:390-395)


def np_thrust(u0):
    """the six thrusts brov_eskf_update_from_solver hands the filter for the solver's input u0 [4]"""
    u = np.asarray(u0, dtype=np.float64)
    return np.array([(-u[0] + u[1] + u[3]) / ROTOR, (-u[0] - u[1] - u[3]) / ROTOR, (u[0] + u[1] - u[3]) / ROTOR, (u[0] - u[1] + u[3]) / ROTOR,
                     -u[2] / ROTOR, -u[2] / ROTOR])
