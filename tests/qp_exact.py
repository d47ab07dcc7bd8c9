"""The QP of one RTI step and its minimiser in far more than double precision: the yardstick of tests/test_qp_exact_cpu.py and
tests/test_gpu_qp_exact.py.

Written from the QP's definition (the comments of oracle/bluerov2_oracle.c), not from any implementation of its solution:

    min  sum_{i<=N} 1/2 dx_i' Qd_i dx_i + q_i' dx_i  +  sum_{i<N} 1/2 du_i' Rd_i du_i + r_i' du_i
    s.t. dx_0 = d0,   dx_{i+1} = A_i dx_i + B_i du_i + b_i,   lb_i <= du_i <= ub_i

    Qd_i = ts_i W[:12] (stage 0: W0 where given), Rd_i = ts_i W[12:], Qd_N = We (unscaled)
    q_i = Qd_i (x_i - yref_i[:12]),  r_i = Rd_i (u_i - yref_i[12:]),  d0 = x0 - x_0,  lb_i = lbu - u_i,  ub_i = ubu - u_i
    multipliers:  Rd du_i + r_i + B_i' pi_i - lam_lo_i + lam_hi_i = 0,   Qd dx_{i+1} + q_{i+1} + A_{i+1}' pi_{i+1} - pi_i = 0
                  (the last one without the A' term), lam >= 0, lam_lo (du - lb) = 0, lam_hi (ub - du) = 0

This is no general QP solver.  With diagonal Rd > 0 and Qd >= 0 the QP is strictly convex, so a point that meets the conditions above IS
the minimiser, and a box-constrained minimiser is fixed by its active set: solve_on(act) is ONE backward Riccati recursion and roll-out
with the inputs of `act` held at their bounds (eliminated, not penalised; the pivot block is at most 4 x 4), certify() evaluates the
optimality conditions in the working precision, and minimiser() repairs a wrong guess one bound at a time.

Every input is taken as the exact value of the double it is given as; arithmetic is mpmath's at 60 digits (model_exact.MpBackend).  Where
mpmath cannot be imported the import error stands: the tests fail, they do not skip."""
import numpy as np

from model_exact import MpBackend, scaled_err  # noqa: F401  (scaled_err: the one error measure of the exact tests)

NX, NU, NY = 12, 4, 16
LOWER, FREE, UPPER = -1, 0, 1
RESIDUAL_TOL = "1e-50"       # relative: dynamics, stationarity, dx_0 = d0
QUANTITIES = ("dx", "du", "pi", "lam", "u0", "cost", "kkt")


class NotCertified(Exception):
    """certify()'s verdict on a point that is not the minimiser: kind 'residual' (an equation does not hold: the solve itself is wrong),
    'bound' (a free input on or outside its box), 'multiplier' (an active multiplier that is not positive).  worst = (stage, input, by how much)"""

    def __init__(self, kind, worst, text):
        super().__init__(f"{kind}: {text}")
        self.kind, self.worst = kind, worst


def _mat(K, a, rows, cols):
    a = np.asarray(a, dtype=np.float64)
    assert a.shape == (rows, cols), (a.shape, rows, cols)
    return [[K.num(v) for v in row] for row in a]


def _vec(K, a, n):
    a = np.asarray(a, dtype=np.float64)
    assert a.shape == (n,), (a.shape, n)
    return [K.num(v) for v in a]


def _solve_spd(H, rhs, zero):
    """H [n][n] symmetric positive definite, n <= 4; rhs: list of n rows of m numbers.  Gaussian elimination without pivoting (every
    leading minor of H is positive); returns X with H X = rhs.  H, rhs are consumed."""
    n = len(H)
    for c in range(n):
        if not H[c][c] > zero:
            raise ArithmeticError("the pivot block is not positive definite")
        for r in range(c + 1, n):
            f = H[r][c] / H[c][c]
            if f == zero:
                continue
            for k in range(c, n):
                H[r][k] -= f * H[c][k]
            rhs[r] = [a - f * b for a, b in zip(rhs[r], rhs[c])]
    for c in range(n - 1, -1, -1):
        for r in range(c + 1, n):
            rhs[c] = [a - H[c][r] * b for a, b in zip(rhs[c], rhs[r])]
        rhs[c] = [a / H[c][c] for a in rhs[c]]
    return rhs


class ExactQP:
    """the QP's data as numbers of the backend K: A [N][12][12], B [N][12][4], b [N][12], Qd, q [N+1][12], Rd, r, lb, ub [N][4], d0 [12]"""

    def __init__(self, K, A, B, b, Qd, q, Rd, r, d0, lb, ub):
        self.K, self.N = K, len(A)
        self.A, self.B, self.b, self.Qd, self.q, self.Rd, self.r, self.d0, self.lb, self.ub = A, B, b, Qd, q, Rd, r, d0, lb, ub
        self.zero = K.lit("0")

    # ---- one equality-constrained solve ---------------------------------------------------------------------------------------------
    def solve_on(self, act):
        """act[i][j] in {LOWER, FREE, UPPER}: the inputs held at a bound.  Returns dict(dx [N+1][12], du [N][4], pi [N][12], lam [N][8]:
        lower | upper, g [N][4] = Rd du + r + B' pi) in the backend's numbers."""
        N, zero = self.N, self.zero
        act = np.asarray(act, dtype=int).reshape(N, NU)
        P = [[self.Qd[N][r] if r == c else zero for c in range(NX)] for r in range(NX)]
        p = list(self.q[N])
        Ps, ps, gains = [None] * (N + 1), [None] * (N + 1), [None] * N
        Ps[N], ps[N] = P, p
        for i in range(N - 1, -1, -1):
            A, B, b = self.A[i], self.B[i], self.b[i]
            F = [j for j in range(NU) if act[i, j] == FREE]
            v = [zero if act[i, j] == FREE else (self.lb[i][j] if act[i, j] == LOWER else self.ub[i][j]) for j in range(NU)]
            c = [b[r] + sum((B[r][j] * v[j] for j in range(NU) if act[i, j] != FREE), zero) for r in range(NX)]
            PA = [[sum((P[r][k] * A[k][cc] for k in range(NX)), zero) for cc in range(NX)] for r in range(NX)]
            Pc = [sum((P[r][k] * c[k] for k in range(NX)), zero) + p[r] for r in range(NX)]
            BF = [[B[k][j] for k in range(NX)] for j in F]                                   # columns of the free inputs
            PB = [[sum((P[r][k] * col[k] for k in range(NX)), zero) for r in range(NX)] for col in BF]
            Huu = [[sum((BF[a][k] * PB[e][k] for k in range(NX)), zero) + (self.Rd[i][F[a]] if a == e else zero) for e in range(len(F))]
                   for a in range(len(F))]
            Hux = [[sum((BF[a][k] * PA[k][cc] for k in range(NX)), zero) for cc in range(NX)] for a in range(len(F))]
            hu = [self.r[i][F[a]] + sum((BF[a][k] * Pc[k] for k in range(NX)), zero) for a in range(len(F))]
            sol = _solve_spd(Huu, [[-h for h in Hux[a]] + [-hu[a]] for a in range(len(F))], zero) if F else []
            Kg, kg = [row[:NX] for row in sol], [row[NX] for row in sol]
            gains[i] = (F, v, Kg, kg)
            if i == 0:
                break     # dx_0 is given: no cost-to-go of stage 0
            Pn = [[sum((A[k][r] * PA[k][cc] for k in range(NX)), zero) + sum((Hux[a][r] * Kg[a][cc] for a in range(len(F))), zero)
                   + (self.Qd[i][r] if r == cc else zero) for cc in range(NX)] for r in range(NX)]
            P = [[(Pn[r][cc] + Pn[cc][r]) / 2 for cc in range(NX)] for r in range(NX)]
            p = [self.q[i][r] + sum((A[k][r] * Pc[k] for k in range(NX)), zero) + sum((Hux[a][r] * kg[a] for a in range(len(F))), zero)
                 for r in range(NX)]
            Ps[i], ps[i] = P, p
        dx, du, pi, lam, g = [list(self.d0)], [], [], [], []
        for i in range(N):
            F, v, Kg, kg = gains[i]
            ui = list(v)
            for a, j in enumerate(F):
                ui[j] = kg[a] + sum((Kg[a][k] * dx[i][k] for k in range(NX)), zero)
            xn = [self.b[i][r] + sum((self.A[i][r][k] * dx[i][k] for k in range(NX)), zero)
                  + sum((self.B[i][r][j] * ui[j] for j in range(NU)), zero) for r in range(NX)]
            du.append(ui); dx.append(xn)
            pi.append([ps[i + 1][r] + sum((Ps[i + 1][r][k] * xn[k] for k in range(NX)), zero) for r in range(NX)])
            gi = [self.Rd[i][j] * ui[j] + self.r[i][j] + sum((self.B[i][k][j] * pi[i][k] for k in range(NX)), zero) for j in range(NU)]
            g.append(gi)
            lam.append([gi[j] if act[i, j] == LOWER else zero for j in range(NU)] + [-gi[j] if act[i, j] == UPPER else zero for j in range(NU)])
        return dict(dx=dx, du=du, pi=pi, lam=lam, g=g)

    # ---- the optimality certificate -----------------------------------------------------------------------------------------------
    def certify(self, sol, act):
        """The conditions that make `sol` THE minimiser, in the working precision: dx_0 = d0, the dynamics and both stationarity equations to
        1e-50 relative (to the largest term of the equation, at least 1); every input held by `act` exactly on its bound with a strictly
        positive multiplier; every other input strictly inside its box with both multipliers zero.  Returns (smallest free slack, smallest
        active multiplier) as floats (inf where there is none); raises NotCertified otherwise."""
        K, N, zero = self.K, self.N, self.zero
        act = np.asarray(act, dtype=int).reshape(N, NU)
        dx, du, pi, lam = sol["dx"], sol["du"], sol["pi"], sol["lam"]
        tol, one = K.lit(RESIDUAL_TOL), K.lit("1")
        worst = zero

        def res(terms):
            nonlocal worst
            s = sum(terms, zero)
            rel = abs(s) / max(one, max(abs(t) for t in terms))
            if rel > worst:
                worst = rel

        for r in range(NX):
            res([dx[0][r], -self.d0[r]])
        for i in range(N):
            for r in range(NX):
                res([dx[i + 1][r], -self.b[i][r]] + [-self.A[i][r][k] * dx[i][k] for k in range(NX)] + [-self.B[i][r][j] * du[i][j] for j in range(NU)])
                t = [self.Qd[i + 1][r] * dx[i + 1][r], self.q[i + 1][r], -pi[i][r]]
                if i + 1 < N:
                    t += [self.A[i + 1][k][r] * pi[i + 1][k] for k in range(NX)]
                res(t)
            for j in range(NU):
                res([self.Rd[i][j] * du[i][j], self.r[i][j], -lam[i][j], lam[i][NU + j]] + [self.B[i][k][j] * pi[i][k] for k in range(NX)])
        if not worst <= tol:
            raise NotCertified("residual", None, f"an equation holds to {float(worst):.1e} relative only")
        slack, mult = None, None
        bad_bound, bad_mult = None, None
        for i in range(N):
            for j in range(NU):
                lo, hi = lam[i][j], lam[i][NU + j]
                if act[i, j] == FREE:
                    if lo != zero or hi != zero:
                        raise NotCertified("residual", (i, j, 0.0), "a free input with a multiplier")
                    s = min(du[i][j] - self.lb[i][j], self.ub[i][j] - du[i][j])
                    slack = s if slack is None or s < slack else slack
                    if not s > zero and (bad_bound is None or s < bad_bound[2]):
                        bad_bound = (i, j, s)
                else:
                    at, m, other = (self.lb[i][j], lo, hi) if act[i, j] == LOWER else (self.ub[i][j], hi, lo)
                    if du[i][j] != at or other != zero:
                        raise NotCertified("residual", (i, j, 0.0), "a held input off its bound, or with the other bound's multiplier")
                    mult = m if mult is None or m < mult else mult
                    if not m > zero and (bad_mult is None or m < bad_mult[2]):
                        bad_mult = (i, j, m)
        if bad_bound is not None or bad_mult is not None:
            e = NotCertified("bound" if bad_bound is not None else "multiplier", bad_bound if bad_bound is not None else bad_mult,
                             f"free input on or outside its box: {_show(bad_bound)}; multiplier not positive: {_show(bad_mult)}")
            e.bad_bound, e.bad_mult = bad_bound, bad_mult
            raise e
        return (float("inf") if slack is None else float(slack)), (float("inf") if mult is None else float(mult))

    def minimiser(self, act_guess, max_rounds=None):
        """solve_on(act_guess), certify; a guess that fails is repaired one round at a time -- the input with the most negative multiplier is
        released, the free input that violates its bound most is held there -- for at most 8 N rounds.  Returns (solution, act, (slack,
        multiplier), rounds) with a certified set, or raises."""
        N = self.N
        act = np.array(act_guess, dtype=int).reshape(N, NU).copy()
        assert np.isin(act, (LOWER, FREE, UPPER)).all()
        for rnd in range((8 * N if max_rounds is None else max_rounds) + 1):
            sol = self.solve_on(act)
            try:
                return sol, act, self.certify(sol, act), rnd
            except NotCertified as e:
                if e.kind == "residual":
                    raise
                if e.bad_mult is not None:
                    act[e.bad_mult[0], e.bad_mult[1]] = FREE
                if e.bad_bound is not None:
                    i, j, _ = e.bad_bound
                    act[i, j] = LOWER if sol["du"][i][j] - self.lb[i][j] <= self.ub[i][j] - sol["du"][i][j] else UPPER
        raise NotCertified("bound", None, f"no certified active set within {8 * N if max_rounds is None else max_rounds} repair rounds")

    def perturbed(self, rng):
        """the same QP with every entry of A, B, b, q, r, d0 multiplied by 1 + s 2^-53, s = +-1 drawn from rng: the data rounded once more"""
        K = self.K
        e = K.lit("2") ** -53

        def pert(a):
            if isinstance(a, list):
                return [pert(v) for v in a]
            return a * (1 + e if rng.integers(0, 2) else 1 - e)
        return ExactQP(K, pert(self.A), pert(self.B), pert(self.b), self.Qd, pert(self.q), self.Rd, pert(self.r), pert(self.d0), self.lb, self.ub)


def _show(w):
    return "none" if w is None else f"stage {w[0]} input {w[1]} by {float(w[2]):.3e}"


def _weights(K, W, We, W0, ts, N):
    W, We = _vec(K, W, NY), _vec(K, We, NX)
    W0 = W if W0 is None else _vec(K, W0, NY)
    ts = _vec(K, np.broadcast_to(np.asarray(ts, dtype=np.float64), (N,)), N)
    return W, We, W0, ts


def build_qp(x, u, x0, yref, W, We, ts, lbu, ubu, A, B, b, W0=None, K=None):
    """the QP of the RTI step that enters at the iterate x [N+1][12], u [N][4] with the given linearisation A, B, b (the caller's: the
    oracle's or the device's), measured state x0, references yref [N+1][16], weights W [16] / We [12] / W0 [16] or None, time steps ts (one
    or N) and input box lbu, ubu"""
    K = K if K is not None else MpBackend()
    N = len(u)
    W, We, W0, ts = _weights(K, W, We, W0, ts, N)
    x, u, yref = _mat(K, x, N + 1, NX), _mat(K, u, N, NU), _mat(K, yref, N + 1, NY)
    x0, lbu, ubu = _vec(K, x0, NX), _vec(K, lbu, NU), _vec(K, ubu, NU)
    Qd, q, Rd, r, lb, ub = [], [], [], [], [], []
    for i in range(N):
        Wi = W0 if i == 0 else W
        Qd.append([ts[i] * Wi[j] for j in range(NX)])
        q.append([Qd[i][j] * (x[i][j] - yref[i][j]) for j in range(NX)])
        Rd.append([ts[i] * Wi[NX + j] for j in range(NU)])
        r.append([Rd[i][j] * (u[i][j] - yref[i][NX + j]) for j in range(NU)])
        lb.append([lbu[j] - u[i][j] for j in range(NU)])
        ub.append([ubu[j] - u[i][j] for j in range(NU)])
    Qd.append(list(We))
    q.append([We[j] * (x[N][j] - yref[N][j]) for j in range(NX)])
    d0 = [x0[j] - x[0][j] for j in range(NX)]
    A = [_mat(K, a, NX, NX) for a in np.asarray(A)]
    B = [_mat(K, a, NX, NU) for a in np.asarray(B)]
    b = [_vec(K, a, NX) for a in np.asarray(b)]
    return ExactQP(K, A, B, b, Qd, q, Rd, r, d0, lb, ub)


def nlp_kkt(qp, u, pi, lam, lbu, ubu):
    """the KKT residual of the ENTERING iterate with its stored multipliers pi [N][12], lam [N][8], as the oracle defines it: the largest
    magnitude among d0, b, the input stationarity r + B' pi - lam_lo + lam_hi, the state stationarity of stages 1 .. N
    (q_i + A_i' pi_i - pi_{i-1}; the last without A'), the bound violations of u and the complementarity products.  qp: build_qp's."""
    K, N, zero = qp.K, qp.N, qp.zero
    u, pi, lam = _mat(K, u, N, NU), _mat(K, pi, N, NX), _mat(K, lam, N, 2 * NU)
    lbu, ubu = _vec(K, lbu, NU), _vec(K, ubu, NU)
    w = max(abs(v) for v in qp.d0)
    for i in range(N):
        w = max([w] + [abs(v) for v in qp.b[i]])
        for c in range(NU):
            w = max(w, abs(qp.r[i][c] - lam[i][c] + lam[i][NU + c] + sum((qp.B[i][k][c] * pi[i][k] for k in range(NX)), zero)))
            sl, su = u[i][c] - lbu[c], ubu[c] - u[i][c]
            w = max(w, -sl, -su, abs(lam[i][c] * sl), abs(lam[i][NU + c] * su))
        if i >= 1:
            for c in range(NX):
                w = max(w, abs(qp.q[i][c] - pi[i - 1][c] + sum((qp.A[i][k][c] * pi[i][k] for k in range(NX)), zero)))
    return max([w] + [abs(qp.q[N][c] - pi[N - 1][c]) for c in range(NX)])


def cost(K, x, u, yref, W, We, ts, W0=None):
    """the least-squares cost of an iterate (x, u: numbers of the backend or doubles): stages scaled by their time step, the terminal one not"""
    N = len(u)
    W, We, W0, ts = _weights(K, W, We, W0, ts, N)
    yref = _mat(K, yref, N + 1, NY)
    c, half = K.lit("0"), K.lit("0.5")
    for i in range(N):
        Wi = W0 if i == 0 else W
        c += half * ts[i] * (sum(Wi[j] * (K.num(x[i][j]) - yref[i][j]) ** 2 for j in range(NX))
                             + sum(Wi[NX + j] * (K.num(u[i][j]) - yref[i][NX + j]) ** 2 for j in range(NU)))
    return c + half * sum(We[j] * (K.num(x[N][j]) - yref[N][j]) ** 2 for j in range(NX))


# ---- double in, double out: one tick of one instance (the entry of the tests' worker processes) ---------------------------------------
def _doubles(K, a):
    return np.array([[K.to_double(v) for v in row] for row in a])


def exact_tick(job):
    """job: dict(x, u, pi, lam: the entering iterate; x0, yref, W, We, W0, ts, lbu, ubu; A, B, b; act: the guessed active set [N][4];
    perturb: seeds of the rounded-data re-solves, or ()).  Returns the certified minimiser and records rounded to double: dict(dx, du, pi,
    lam, u0, cost, kkt, x, u: the new iterate, act, slack, mult, rounds, D: {quantity: largest scaled difference of the re-solves})."""
    K = MpBackend()
    N = len(job["u"])
    args = (job["x0"], job["yref"], job["W"], job["We"], job["ts"], job["lbu"], job["ubu"], job["A"], job["B"], job["b"])
    qp = build_qp(job["x"], job["u"], *args, W0=job.get("W0"), K=K)
    sol, act, (slack, mult), rounds = qp.minimiser(job["act"])
    out = _round(K, qp, sol, job)
    out.update(act=act, slack=slack, mult=mult, rounds=rounds, D={})
    for seed in job.get("perturb", ()):
        alt = qp.perturbed(np.random.default_rng(seed))
        other = _round(K, alt, alt.solve_on(act), job)
        for k in QUANTITIES:
            out["D"][k] = max(out["D"].get(k, 0.0), float(np.max(scaled_err(other[k], out[k]))))
    return out


def _round(K, qp, sol, job):
    N = qp.N
    xn = [[K.num(job["x"][i][j]) + sol["dx"][i][j] for j in range(NX)] for i in range(N + 1)]
    un = [[K.num(job["u"][i][j]) + sol["du"][i][j] for j in range(NU)] for i in range(N)]
    return dict(dx=_doubles(K, sol["dx"]), du=_doubles(K, sol["du"]), pi=_doubles(K, sol["pi"]), lam=_doubles(K, sol["lam"]),
                x=_doubles(K, xn), u=_doubles(K, un), u0=np.array([K.to_double(v) for v in un[0]]),
                cost=K.to_double(cost(K, xn, un, job["yref"], job["W"], job["We"], job["ts"], job.get("W0"))),
                kkt=K.to_double(nlp_kkt(qp, job["u"], job["pi"], job["lam"], job["lbu"], job["ubu"])))
