"""The cases of the exact QP tests (tests/test_qp_exact_cpu.py, tests/test_gpu_qp_exact.py): seeded draws, few instances, short horizons.

A ROW is one kernel instantiation: (N, Ts, kernel_path, B, environment, kind of the LDS kernel, stages per window, extra).  The LDS-resident
rows are LIN's of tests/test_gpu_model_exact.py -- the smallest shapes that reach each instantiation -- with B held to 4 (2 at N = 80),
then N = 24 (the first horizon past the fused kernels), N = 129 (the first of rti_window_kernel_long), the streaming pair at N = 4, 20,
40, a geometric time grid with a stage-0 weight, and the 6-disturbance model.

Every row runs four KINDS of instance for two ticks, tick 2 entering from tick 1's exact minimiser:
    a   no bound active: the early exit (qp_iter == 0)
    b   the same instances with qp_early_exit = 0: the interior-point loop on a QP without active bounds
    c   a tight box (+-6 .. +-12), a start metres off and a terminal reference whose velocities are metres per second off: bounds active at
        stage 0, at stage N - 1 and on both sides of a window / wave seam
    d   a box that excludes 0 on one input (lbu[1], ubu[1] = 2, 30): the entering iterate is infeasible
The conditions are asserted by `hold_kind` wherever a case is solved, with the oracle's linearisation on the CPU and with the device's on
the GPU, together with the margins every case must have: every active multiplier and every free slack of the certified minimiser above
1e-6.  A draw that does not meet them is replaced HERE (SEEDS; `python tests/qp_exact_cases.py` searches); nothing is dropped at run time."""
import collections
import os

import numpy as np

from qp_exact import FREE, LOWER, NU, NX, UPPER, scaled_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICKS = 2
MARGIN = 1e-6
PI_MAX = 1e6
ORACLE_CEILING = 1e-10     # four times the oracle's worst scaled error against the certified minimiser stays below this
KINDS = ("a", "b", "c", "d")
P_NOMINAL = np.array([0, 0, 0, 0, 1.7182, 0, 5.468, 0.4006, -11.7391, -20, -31.8678, -5, -18.18, -21.66, -36.99, -1.55])

Row = collections.namedtuple("Row", "N Ts path B env kind win extra")
ROWS = [
    Row(4, 0.05, 2, 4, {}, "fused*", None, ""),
    Row(10, 0.1, 2, 4, {}, "fused, two waves per SIMD", None, ""),
    Row(20, 0.05, 2, 3, {}, "fused", None, ""),
    Row(40, 0.0125, 2, 2, {}, "windowed, resident", 40, ""),                                  # four waves, a quarter of the horizon each
    Row(40, 0.0125, 2, 3, {"BROV_DEV_WIN_BLOCKS": "1"}, "windowed, resident", 40, ""),      # ... one block for all three instances
    Row(40, 0.0125, 2, 2, {"BROV_DEV_NO_RESIDENT": "1"}, "windowed", 20, ""),               # windows of 20 stages
    Row(80, 0.0125, 2, 2, {}, "windowed, resident", 80, ""),
    Row(24, 0.0125, 2, 2, {}, "windowed, resident", 24, ""),                                    # the first horizon past the fused kernels
    Row(129, 0.0125, 2, 1, {}, "windowed", 19, ""),                                           # rti_window_kernel_long: seven windows of <= 19
    Row(4, 0.05, 1, 4, {}, None, None, ""), Row(20, 0.05, 1, 3, {}, None, None, ""), Row(40, 0.0125, 1, 2, {}, None, None, ""),
    Row(20, 0.0125, 2, 2, {}, "fused", None, "grid"),                                         # geometric grid 0.0125 .. 0.1, stage-0 weight
    Row(20, 0.05, 2, 2, {}, "fused", None, "dist6"),                                          # roll / pitch moments in the model
]


def row_name(row):
    return f"N={row.N} path={row.path} B={row.B} {row.kind or 'streaming'}" + (" " + ",".join(row.env) if row.env else "") + (" " + row.extra if row.extra else "")


def seams(row):
    """the stages s whose pair (s - 1, s) straddles a seam: window boundaries of the windowed kernel, the four waves' quarters of the resident one"""
    if row.win is None:
        return []
    step = (row.N + 3) // 4 if row.win == row.N else row.win
    return list(range(step, row.N, step))


# (row index, kind) -> the seeds of its B instances.  Kind b runs kind a's.
SEEDS = {}


def seeds_of(r, kind):
    return SEEDS[(r, "a" if kind == "b" else kind)]


def _circle():
    c = np.load(os.path.join(ROOT, "tests", "golden", "traj_head.npz"))["circle"]
    return np.concatenate([c, np.repeat(c[-1:], 160, axis=0)])


def box(r, kind):
    """the input box of a (row, kind): one per solver"""
    rng = np.random.default_rng(7000 + 10 * r + KINDS.index(kind))
    lbu, ubu = np.full(4, -50.0), np.full(4, 50.0)
    if kind == "c":
        lbu, ubu = -rng.uniform(6, 12, 4), rng.uniform(6, 12, 4)
    if kind == "d":
        lbu[1], ubu[1] = 2.0, 30.0
    return lbu, ubu


def instance(r, kind, seed):
    """one instance's inputs: dict(x0 [12], x [N+1][12], u [N][4], p [N+1][16], rp [N+1][2] or None, yrefs [TICKS][N+1][16])"""
    row = ROWS[r]
    N = row.N
    rng = np.random.default_rng(seed)
    circ = _circle()
    yrefs = [circ[2 * k:2 * k + N + 1].copy() for k in range(TICKS)]
    x = yrefs[0][:, :NX] + rng.normal(size=(N + 1, NX)) * 0.01
    u = rng.normal(size=(N, NU)) * 0.5
    x0 = x[0] + rng.normal(size=NX) * 0.01
    p = np.tile(P_NOMINAL, (N + 1, 1))
    p[:, 4:] *= rng.uniform(0.9, 1.1, size=12)
    p[:, :4] = rng.uniform(-2, 2, size=4)
    if kind == "c":      # metres off
        x0[:3] += rng.uniform(2.0, 4.0, size=3) * rng.choice([-1.0, 1.0], size=3)
        x0[5] += rng.uniform(-0.3, 0.3)
        # ... and a terminal reference whose velocities differ by metres per second: what the last stages' inputs are spent on
        dv = rng.uniform(2.0, 5.0, size=3) * rng.choice([-1.0, 1.0], size=3)
        for y in yrefs:
            y[N, 6:9] += dv
    if kind == "d":
        x0[:3] += rng.uniform(-0.3, 0.3, size=3)
    rp = np.tile(rng.uniform(-1, 1, size=2), (N + 1, 1)) if row.extra == "dist6" else None
    return dict(x0=x0, x=x, u=u, p=p, rp=rp, yrefs=yrefs)


def grid(row, W):
    """(ts [N], W0 or None): the geometric grid and stage-0 weight of the row that has them"""
    if row.extra != "grid":
        return np.full(row.N, row.Ts), None
    return row.Ts * 8.0 ** (np.arange(row.N) / (row.N - 1.0)), np.asarray(W) * np.linspace(0.5, 2.0, 16)


# ---- the oracle's side, in double -------------------------------------------------------------------------------------------------------
def oracle_linearisation(orc, x, u, p, ts, rp):
    """A, B, b as orc_rti_step forms them (rti_step(..., want_lin=True) gives the same for the shipped model; this also takes the moments)"""
    N = len(u)
    A, B, b = np.empty((N, NX, NX)), np.empty((N, NX, NU)), np.empty((N, NX))
    for i in range(N):
        xn, A[i], B[i] = orc.rk4_sens(x[i], u[i], p[i], float(ts[i]), None if rp is None else rp[i])
        b[i] = xn - x[i + 1]
    return A, B, b


def qp_data_double(x, u, x0, yref, W, We, ts, lbu, ubu, W0=None):
    """Qd, q, Rd, r, d0, lb, ub in double, operation by operation as orc_rti_step_ws forms them"""
    N = len(u)
    Wst = np.tile(np.asarray(W, dtype=float), (N, 1))
    if W0 is not None:
        Wst[0] = W0
    Qd = np.concatenate([ts[:, None] * Wst[:, :NX], np.asarray(We, dtype=float)[None]])
    q = Qd * (x - yref[:, :NX])
    Rd = ts[:, None] * Wst[:, NX:]
    r = Rd * (u - yref[:N, NX:])
    return Qd, q, Rd, r, x0 - x[0], lbu[None] - u, ubu[None] - u


def kkt_double(A, B, b, q, r, d0, u, pi, lam, lbu, ubu):
    """the entering iterate's KKT residual in double, term by term in the oracle's order"""
    N = len(u)
    w = float(np.abs(d0).max())
    for i in range(N):
        w = max(w, float(np.abs(b[i]).max()))
        for c in range(NU):
            s = r[i, c] - lam[i, c] + lam[i, 4 + c]
            for k in range(NX):
                s += B[i, k, c] * pi[i, k]
            sl, su = u[i, c] - lbu[c], ubu[c] - u[i, c]
            w = max(w, abs(s), -sl, -su, abs(lam[i, c] * sl), abs(lam[i, 4 + c] * su))
        if i >= 1:
            for c in range(NX):
                s = q[i, c] - pi[i - 1, c]
                for k in range(NX):
                    s += A[i, k, c] * pi[i, k]
                w = max(w, abs(s))
    return max(w, float(np.abs(q[N] - pi[N - 1]).max()))


def cost_double(x, u, yref, W, We, ts, W0=None):
    """the cost in double, accumulated term by term in the oracle's order"""
    N, c = len(u), 0.0
    for i in range(N):
        Wi = W0 if (i == 0 and W0 is not None) else W
        for j in range(NX):
            e = x[i, j] - yref[i, j]
            c += 0.5 * ts[i] * Wi[j] * e * e
        for j in range(NU):
            e = u[i, j] - yref[i, NX + j]
            c += 0.5 * ts[i] * Wi[NX + j] * e * e
    for j in range(NX):
        e = x[N, j] - yref[N, j]
        c += 0.5 * We[j] * e * e
    return c


def guess_from(du, lb, ub):
    """the active set a double-precision answer sits on: inputs on (within 1e-9 of) a bound"""
    act = np.full(du.shape, FREE, dtype=int)
    act[du - lb <= 1e-9 * np.maximum(1.0, np.abs(lb))] = LOWER
    act[ub - du <= 1e-9 * np.maximum(1.0, np.abs(ub))] = UPPER
    return act


def oracle_tick(orc, opts, A, B, b, x, u, pi, lam, x0, yref, W, We, ts, lbu, ubu, W0):
    """oracle.qp_solve on the given linearisation, its full step as orc_rti_step takes it, and the records in double.  Returns dict(dx, du:
    the new iterate minus the entering one; pi, lam, u0, cost, kkt; act: the active-set guess; status, iters, early)"""
    Qd, q, Rd, r, d0, lb, ub = qp_data_double(x, u, x0, yref, W, We, ts, lbu, ubu, W0)
    o = orc.qp_solve(opts, A, B, b, Qd, q, Rd, r, d0, lb, ub)
    xn, un = x + o["dx"], u + o["du"]
    return dict(dx=xn - x, du=un - u, pi=o["pi"], lam=o["lam"], u0=un[0].copy(), cost=cost_double(xn, un, yref, W, We, ts, W0),
                kkt=kkt_double(A, B, b, q, r, d0, u, pi, lam, lbu, ubu), act=guess_from(o["du"], lb, ub), status=o["status"],
                iters=o["iters"], early=o["early"])


def errors(got, ref):
    """{quantity: worst scaled error} of an answer (dict(dx, du, pi, lam, u0, cost, kkt)) against exact_tick's"""
    return {k: float(np.max(scaled_err(got[k], ref[k]))) for k in ("dx", "du", "pi", "lam", "u0", "cost", "kkt")}


def hold_kind(row, kind, tick, ex, lb, ub, early=None):
    """the conditions of the case's kind on its certified minimiser `ex` (exact_tick's), asserted: the margins, and what must be active.
    early: whether the double-precision solver took the early exit (kind a: it must)."""
    act = ex["act"]
    N = row.N
    assert ex["slack"] > MARGIN and ex["mult"] > MARGIN, (row_name(row), kind, tick, "margins", ex["slack"], ex["mult"])
    # (a start so far off that the full step has left the model's range -- quadratic damping beyond what one ERK4 step integrates stably,
    # sensitivities and multipliers of 1e10 and more -- says nothing about the QP layer: the suite's other tests stop at KKT 1e6 as well)
    assert np.abs(ex["pi"]).max() <= PI_MAX and ex["kkt"] <= PI_MAX, (row_name(row), kind, tick, "diverged", np.abs(ex["pi"]).max(), ex["kkt"])
    n_act = int((act != FREE).sum())
    if kind in ("a", "b"):
        assert n_act == 0, (row_name(row), kind, tick, "bounds active", n_act)
        if kind == "a" and early is not None:
            assert early, (row_name(row), kind, tick, "no early exit")
    if kind == "c":
        assert n_act >= 3 and (act == FREE).any(), (row_name(row), kind, tick, n_act)
        if tick == 0:
            assert (act[0] != FREE).any() and (act[N - 1] != FREE).any(), (row_name(row), kind, "no bound active at stage 0 / N - 1")
            ss = seams(row)
            assert not ss or any((act[s - 1] != FREE).any() and (act[s] != FREE).any() for s in ss), (row_name(row), kind, "no seam with a bound active on either side")
    if kind == "d" and tick == 0:
        assert (lb > 0).any() or (ub < 0).any(), (row_name(row), kind, "the entering iterate is feasible")
        assert n_act >= 1
    return n_act


def job_of(x, u, pi, lam, x0, yref, W, We, W0, ts, lbu, ubu, A, B, b, act, perturb=()):
    return dict(x=x, u=u, pi=pi, lam=lam, x0=x0, yref=yref, W=np.asarray(W, dtype=float), We=np.asarray(We, dtype=float), W0=W0, ts=ts,
                lbu=lbu, ubu=ubu, A=A, B=B, b=b, act=act, perturb=tuple(perturb))


def oracle_options(orc, row, kind):
    lbu, ubu = box(ROWS.index(row), kind)
    o = orc.opts(row.N, row.Ts, lbu=lbu, ubu=ubu, qp_early_exit=0 if kind == "b" else 1)
    W, We = np.array(o.W[:]), np.array(o.We[:])
    ts, W0 = grid(row, W)
    if row.extra == "grid":
        o = orc.opts(row.N, row.Ts, lbu=lbu, ubu=ubu, qp_early_exit=0 if kind == "b" else 1, ts_vec=ts, W0=W0)
    return o, W, We, ts, W0, lbu, ubu


def cpu_case(orc, r, kind, seed, exact, ticks=TICKS):
    """one instance through `ticks` ticks on the oracle's own linearisation.  exact: callable(job) -> exact_tick's result.  Returns per tick
    dict(ex: the certified minimiser, orc: the oracle's answer, err: the oracle's errors, n_act); asserts the kind's conditions."""
    row = ROWS[r]
    o, W, We, ts, W0, lbu, ubu = oracle_options(orc, row, kind)
    ins = instance(r, kind, seed)
    x, u = ins["x"].copy(), ins["u"].copy()
    pi, lam = np.zeros((row.N, NX)), np.zeros((row.N, 8))
    out = []
    for k in range(ticks):
        A, B, b = oracle_linearisation(orc, x, u, ins["p"], ts, ins["rp"])
        ot = oracle_tick(orc, o, A, B, b, x, u, pi, lam, ins["x0"], ins["yrefs"][k], W, We, ts, lbu, ubu, W0)
        assert ot["status"] == 0, (row_name(row), kind, seed, k, ot["status"])
        ex = exact(job_of(x, u, pi, lam, ins["x0"], ins["yrefs"][k], W, We, W0, ts, lbu, ubu, A, B, b, ot["act"]))
        n_act = hold_kind(row, kind, k, ex, lbu[None] - u, ubu[None] - u, early=ot["early"])
        out.append(dict(ex=ex, orc=ot, err=errors(ot, ex), n_act=n_act, lin=(A, B, b)))
        x, u, pi, lam = ex["x"], ex["u"], ex["pi"], ex["lam"]
    return out


def cpu_case_job(args):
    """worker entry (process pool): cpu_case of (row index, kind, seed) with an oracle of the worker's own; per tick dict(err, slack, mult,
    n_act, rounds, iters, act, x, u: the exact new iterate)"""
    from oracle.oracle_ffi import Oracle
    from qp_exact import exact_tick
    r, kind, seed = args
    return [dict(err=t["err"], slack=t["ex"]["slack"], mult=t["ex"]["mult"], n_act=t["n_act"], rounds=t["ex"]["rounds"], iters=t["orc"]["iters"],
                 act=t["ex"]["act"], x=t["ex"]["x"], u=t["ex"]["u"]) for t in cpu_case(Oracle(), r, kind, seed, exact_tick)]


def _search_one(args):
    from qp_exact import NotCertified
    r, kind, seed = args
    try:
        res = cpu_case_job(args)
        assert all(4.0 * max(t["err"].values()) < ORACLE_CEILING for t in res), ("oracle ceiling", [max(t["err"].values()) for t in res])
        return r, kind, seed, True, [(t["slack"], t["mult"], t["n_act"], t["rounds"]) for t in res]
    except (AssertionError, NotCertified, ArithmeticError) as e:
        return r, kind, seed, False, str(e)[:200]


def search(tries=12, first=0, kinds=("a", "c", "d")):
    """for every (row, kind) the first seeds that meet the kind's conditions on the CPU; prints the SEEDS table"""
    import concurrent.futures
    import multiprocessing
    found = {}
    with concurrent.futures.ProcessPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)))), mp_context=multiprocessing.get_context("spawn")) as pool:
        for r, row in enumerate(ROWS):
            if r < first:
                continue
            for kind in kinds:
                base = 100000 * (r + 1) + 1000 * KINDS.index(kind)
                good, start = [], 0
                while len(good) < row.B and start < 20 * tries:
                    for _, _, seed, ok, info in pool.map(_search_one, [(r, kind, base + s) for s in range(start, start + tries)]):
                        if ok and len(good) < row.B:
                            good.append(seed)
                            print(f"# {row_name(row)} {kind} seed {seed}: (slack, multiplier, active, repair rounds) per tick {info}", flush=True)
                    start += tries
                assert len(good) == row.B, (row_name(row), kind, "no draw found")
                found[(r, kind)] = good
                print(f"    ({r}, {kind!r}): {good},", flush=True)
    return found


SEEDS.update({
    (0, 'a'): [100000, 100001, 100002, 100003],
    (0, 'c'): [102000, 102001, 102002, 102003],
    (0, 'd'): [103000, 103001, 103002, 103003],
    (1, 'a'): [200000, 200001, 200002, 200003],
    (1, 'c'): [202002, 202003, 202004, 202005],
    (1, 'd'): [203000, 203001, 203002, 203003],
    (2, 'a'): [300000, 300001, 300002],
    (2, 'c'): [302000, 302001, 302002],
    (2, 'd'): [303000, 303001, 303002],
    (3, 'a'): [400000, 400001],
    (3, 'c'): [402000, 402001],
    (3, 'd'): [403000, 403001],
    (4, 'a'): [500000, 500001, 500002],
    (4, 'c'): [502000, 502001, 502002],
    (4, 'd'): [503000, 503001, 503002],
    (5, 'a'): [600000, 600001],
    (5, 'c'): [602000, 602002],
    (5, 'd'): [603000, 603001],
    (6, 'a'): [700000, 700001],
    (6, 'c'): [702001, 702003],
    (6, 'd'): [703000, 703001],
    (7, 'a'): [800000, 800001],
    (7, 'c'): [802000, 802001],
    (7, 'd'): [803000, 803001],
    (8, 'a'): [900000],
    (8, 'c'): [902000],
    (8, 'd'): [903000],
    (9, 'a'): [1000000, 1000001, 1000002, 1000003],
    (9, 'c'): [1002000, 1002001, 1002002, 1002003],
    (9, 'd'): [1003000, 1003001, 1003002, 1003003],
    (10, 'a'): [1100000, 1100001, 1100002],
    (10, 'c'): [1102000, 1102001, 1102002],
    (10, 'd'): [1103000, 1103001, 1103002],
    (11, 'a'): [1200000, 1200001],
    (11, 'c'): [1202000, 1202001],
    (11, 'd'): [1203000, 1203001],
    (12, 'a'): [1300000, 1300001],
    (12, 'c'): [1302003, 1302005],
    (12, 'd'): [1303000, 1303001],
    (13, 'a'): [1400000, 1400001],
    (13, 'c'): [1402000, 1402001],
    (13, 'd'): [1403000, 1403001],
})


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    search(first=int(sys.argv[1]) if len(sys.argv) > 1 else 0, kinds=tuple(sys.argv[2]) if len(sys.argv) > 2 else ("a", "c", "d"))
