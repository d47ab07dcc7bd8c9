"""The BlueROV2 model, one ERK4 step and its sensitivities in far more than double precision: the yardstick of
tests/test_model_exact_cpu.py and tests/test_gpu_model_exact.py.

Written from the model's equations (bluerov2.py: thruster map, propulsion matrix, the twelve rows incl. the sin(psi) term of
dphi) and the comments of bluerov2_amd/csrc/bluerov2_model.hpp (world-frame wrench projected with R^T at every stage, the two
roll / pitch moments of the 6-disturbance variant entering dp, dq), not from any other implementation:

    f(x, u, p, ww, rp)           the twelve rows
    erk4(x, u, p, h, ...)        one explicit RK4 step; `substeps` of them over h with substeps=
    sens(x, u, p, h, ...)        S = d x+ / d [x; u] by central differences at a step far below the working precision

Every input is taken as the exact value of the double it is given as; the model's constants are its decimal literals (0.707 is
707/1000, not the double nearest to it).  The body uses sin, cos, abs and arithmetic only, through a small backend, so that it
runs on mpmath (60 digits, the reference) and on numpy.longdouble (x87: 64-bit mantissa; good for f and x+, not for S).

|v| v is abs(v) * v: at v = 0 the central difference straddles the kink and gives the step itself, 1e-25, where the model's
convention d|v|v/dv = 2|v| gives 0 -- the same number at every precision this is compared at.
"""
import numpy as np

NX, NU, NP = 12, 4, 16
DIGITS = 60
FD_STEP = "1e-25"     # central differences: truncation ~ step^2 = 1e-50 relative, cancellation 10^(25 - 60)


class MpBackend:
    name = "mpmath"

    def __init__(self, digits=DIGITS):
        import mpmath
        self.mp = mpmath.mp.clone()
        self.mp.dps = int(digits)
        self.sin, self.cos = self.mp.sin, self.mp.cos
        self.abs = abs

    def num(self, v):
        """the exact value of a double (or a number of this backend, unchanged)"""
        return v if isinstance(v, self.mp.mpf) else self.mp.mpf(float(v))

    def lit(self, s):
        return self.mp.mpf(s)

    def to_double(self, v):
        return float(v)      # mpmath rounds to nearest


class LongDoubleBackend:
    name = "longdouble"

    def __init__(self):
        if np.finfo(np.longdouble).nmant < 63:
            raise RuntimeError("numpy.longdouble has no more mantissa than double here: no high-precision reference")
        self.sin, self.cos, self.abs = np.sin, np.cos, np.abs

    def num(self, v):
        return np.longdouble(v)

    def lit(self, s):
        return np.longdouble(s)

    def to_double(self, v):
        return float(v)


def backend(allow_longdouble=True):
    """mpmath at 60 digits; where it cannot be imported, numpy.longdouble with a 64-bit mantissa; else an error (never a skip)"""
    try:
        return MpBackend()
    except ImportError:
        if not allow_longdouble:
            raise
        return LongDoubleBackend()


class ExactModel:
    def __init__(self, K=None):
        self.K = K = K if K is not None else MpBackend()
        L = K.lit
        self.m, self.Ix, self.Iy, self.Iz = L("11.26"), L("0.3"), L("0.63"), L("0.58")
        self.ZG, self.g, self.bouy = L("0.02"), L("9.81"), L("0.66")
        self.rotor = L("0.026546960744430276")
        self.k707, self.k167, self.k175 = L("0.707"), L("0.167"), L("0.175")
        self.half, self.two, self.six = L("0.5"), L("2"), L("6")
        self.zero = L("0")

    def vec(self, a, n=None):
        a = list(a) if not isinstance(a, np.ndarray) else list(a.ravel())
        assert n is None or len(a) == n, (len(a), n)
        return [self.K.num(v) for v in a]

    def f(self, x, u, p, ww=None, rp=None):
        """the twelve rows; x, u, p (and ww[6] world-frame wrench, rp[2] roll / pitch moments) numbers of the backend"""
        K = self
        sin, cos, ab = self.K.sin, self.K.cos, self.K.abs
        ph, th, ps, vu, vv, vw, wp, wq, wr = x[3], x[4], x[5], x[6], x[7], x[8], x[9], x[10], x[11]
        sph, cph, sth, cth, sps, cps = sin(ph), cos(ph), sin(th), cos(th), sin(ps), cos(ps)
        # body -> world rotation of the kinematic rows
        R = [[cps * cth, -sps * cph + cps * sth * sph, sps * sph + cps * cph * sth],
             [sps * cth, cps * cph + sph * sth * sps, -cps * sph + sth * sps * cph],
             [-sth, cth * sph, cth * cph]]
        t0 = (-u[0] + u[1] + u[3]) / K.rotor
        t1 = (-u[0] - u[1] - u[3]) / K.rotor
        t2 = (u[0] + u[1] - u[3]) / K.rotor
        t3 = (u[0] - u[1] + u[3]) / K.rotor
        t4 = -u[2] / K.rotor
        t5 = -u[2] / K.rotor
        Kt0 = K.k707 * t0 + K.k707 * t1 - K.k707 * t2 - K.k707 * t3
        Kt1 = K.k707 * t0 - K.k707 * t1 + K.k707 * t2 - K.k707 * t3
        Kt2 = t4 + t5
        Kt3, Kt4 = K.zero, K.zero
        Kt5 = K.k167 * t0 - K.k167 * t1 - K.k175 * t2 + K.k175 * t3
        dx, dy, dz, dn = p[0], p[1], p[2], p[3]
        if rp is not None:
            Kt3, Kt4 = Kt3 + rp[0], Kt4 + rp[1]
        if ww is not None:
            # f_b = R^T f_w, t_b = R^T t_w with THIS point's attitude, entering where the model's own disturbances do
            fb = [R[0][j] * ww[0] + R[1][j] * ww[1] + R[2][j] * ww[2] for j in range(3)]
            tb = [R[0][j] * ww[3] + R[1][j] * ww[4] + R[2][j] * ww[5] for j in range(3)]
            dx, dy, dz = dx + fb[0], dy + fb[1], dz + fb[2]
            Kt3, Kt4, dn = Kt3 + tb[0], Kt4 + tb[1], dn + tb[2]
        o = [None] * NX
        for i in range(3):
            o[i] = R[i][0] * vu + R[i][1] * vv + R[i][2] * vw
        o[3] = wp + (sps * sth / cth) * wq + cph * sth / cth * wr      # sin(psi): as the model has it
        o[4] = cph * wq + sph * wr
        o[5] = (sph / cth) * wq + (cph / cth) * wr
        o[6] = (Kt0 - K.bouy * sth + dx + p[8] * vu + p[12] * ab(vu) * vu) / (K.m + p[4])
        o[7] = (Kt1 + K.bouy * cth * sph + dy + p[9] * vv + p[13] * ab(vv) * vv) / (K.m + p[5])
        o[8] = (Kt2 + K.bouy * cth * cph + dz + p[10] * vw + p[14] * ab(vw) * vw) / (K.m + p[6])
        o[9] = (Kt3 + (K.Iy - K.Iz) * wq * wr - K.m * K.ZG * K.g * cth * sph) / K.Ix
        o[10] = (Kt4 + (K.Iz - K.Ix) * wp * wr - K.m * K.ZG * K.g * sth) / K.Iy
        o[11] = (Kt5 - (K.Iy - K.Ix) * wp * wq + dn + p[11] * wr + p[15] * ab(wr) * wr) / (K.Iz + p[7])
        return o

    def _step(self, x, u, p, h, ww, rp):
        f = self.f
        k1 = f(x, u, p, ww, rp)
        k2 = f([a + self.half * h * b for a, b in zip(x, k1)], u, p, ww, rp)
        k3 = f([a + self.half * h * b for a, b in zip(x, k2)], u, p, ww, rp)
        k4 = f([a + h * b for a, b in zip(x, k3)], u, p, ww, rp)
        return [a + h / self.six * (b + self.two * c + self.two * d + e) for a, b, c, d, e in zip(x, k1, k2, k3, k4)]

    def _erk4(self, x, u, p, h, ww, rp, substeps):
        hs = h / self.K.num(substeps)
        for _ in range(int(substeps)):
            x = self._step(x, u, p, hs, ww, rp)
        return x

    def _args(self, x, u, p, h, ww, rp):
        return (self.vec(x, NX), self.vec(u, NU), self.vec(p, NP), self.K.num(h), None if ww is None else self.vec(ww, 6),
                None if rp is None else self.vec(rp, 2))

    # ---- double in, double out ---------------------------------------------------------------------------------------------
    def f_double(self, x, u, p, ww=None, rp=None):
        x, u, p, _, ww, rp = self._args(x, u, p, 0.0, ww, rp)
        return np.array([self.K.to_double(v) for v in self.f(x, u, p, ww, rp)])

    def erk4(self, x, u, p, h, ww=None, rp=None, substeps=1):
        """x+ after `substeps` ERK4 steps of h / substeps, rounded to double"""
        x, u, p, h, ww, rp = self._args(x, u, p, h, ww, rp)
        return np.array([self.K.to_double(v) for v in self._erk4(x, u, p, h, ww, rp, substeps)])

    def jac(self, x, u, p, ww=None, rp=None):
        """[df/dx | df/du] [12][16], rounded to double; central differences (mpmath only)"""
        return self._diff(lambda xx, uu, pp, hh, w, r: self.f(xx, uu, pp, w, r), x, u, p, 0.0, ww, rp)[1]

    def _diff(self, fun, x, u, p, h, ww, rp):
        assert self.K.name == "mpmath", "derivatives by differences need the 60-digit backend"
        x, u, p, h, ww, rp = self._args(x, u, p, h, ww, rp)
        e = self.K.lit(FD_STEP)
        J = np.empty((NX, NX + NU))
        z = x + u
        for c in range(NX + NU):
            zp, zm = list(z), list(z)
            zp[c], zm[c] = z[c] + e, z[c] - e
            dp_, dm_ = fun(zp[:NX], zp[NX:], p, h, ww, rp), fun(zm[:NX], zm[NX:], p, h, ww, rp)
            J[:, c] = [self.K.to_double((a - b) / (self.two * e)) for a, b in zip(dp_, dm_)]
        return np.array([self.K.to_double(v) for v in fun(x, u, p, h, ww, rp)]), J

    def sens(self, x, u, p, h, ww=None, rp=None, substeps=1):
        """(x+ [12], S [12][16] = d x+ / d [x; u]), rounded to double; central differences (mpmath only: see the module text)"""
        return self._diff(lambda xx, uu, pp, hh, w, r: self._erk4(xx, uu, pp, hh, w, r, substeps), x, u, p, h, ww, rp)


def scaled_err(got, ref):
    """|got - ref| / max(1, |ref|), entry by entry (NaN where got is NaN)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


def ulp_err(got, exact_mp, mp):
    """|got - exact| in units of the last place of the double nearest to exact (exact: an mpf)"""
    import math
    ref = float(exact_mp)
    if ref == 0.0:
        return 0.0 if got == 0.0 else math.inf
    u = math.ulp(ref)
    return float(abs(mp.mpf(float(got)) - exact_mp) / mp.mpf(u))
