"""The exact QP reference (tests/qp_exact.py) against itself, and the double-precision oracle against it, without a GPU.

1. solve_on against a dense 60-digit solve of the whole KKT system (mpmath.lu_solve) at N = 2 and 3 on random data, to 1e-50; certify
   rejects an active set with one bound too many and one with one too few; the repair loop finds the certified set from the empty guess.
2. Every case of tests/qp_exact_cases.py, both ticks, on the oracle's own linearisation: the kind's conditions and the margins are
   asserted and printed, and the oracle's scaled errors against the certified minimiser are recorded per quantity.  Their ceiling --
   four times the worst stays below 1e-10 -- is what keeps the GPU test's bar (4 x the oracle's error) meaningful.
3. The independent recipe (scripts/make_golden.py: the reference's CasADi model, numpy condensing, scipy BVLS) at N = 20: its u against the
   certified minimiser, at its own 1e-9."""
import concurrent.futures
import multiprocessing
import os
import sys

import numpy as np
import pytest

import qp_exact_cases as C
from qp_exact import FREE, LOWER, NU, NX, UPPER, ExactQP, MpBackend, NotCertified, exact_tick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_CEILING = C.ORACLE_CEILING


@pytest.fixture(scope="module")
def pool():
    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    p = concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn"))
    yield p
    p.shutdown()


# ---- 1. the exact solver against itself ---------------------------------------------------------------------------------------------
def _random_qp(K, N, rng):
    num = lambda a: [[K.num(v) for v in row] for row in a]
    A = [num(np.eye(NX) + 0.3 * rng.normal(size=(NX, NX))) for _ in range(N)]
    B = [num(rng.normal(size=(NX, NU))) for _ in range(N)]
    b = num(rng.normal(size=(N, NX)))
    Qd, q = num(rng.uniform(0.1, 10.0, size=(N + 1, NX))), num(rng.normal(size=(N + 1, NX)) * 3)
    Rd, r = num(rng.uniform(0.01, 1.0, size=(N, NU))), num(rng.normal(size=(N, NU)))
    lb, ub = num(-rng.uniform(0.5, 2.0, size=(N, NU))), num(rng.uniform(0.5, 2.0, size=(N, NU)))
    return ExactQP(K, A, B, b, Qd, q, Rd, r, [K.num(v) for v in rng.normal(size=NX)], lb, ub)


def _dense_solve(qp, act):
    """the KKT system of the equality-constrained QP as ONE linear system in (dx_0 .. dx_N, the free du, pi_{-1}, pi_0 .. pi_{N-1}), solved
    by mpmath's LU; returns dx, du, pi, g like solve_on"""
    mp, N, zero = qp.K.mp, qp.N, qp.zero
    free = [(i, j) for i in range(N) for j in range(NU) if act[i, j] == FREE]
    held = {(i, j): (qp.lb[i][j] if act[i, j] == LOWER else qp.ub[i][j]) for i in range(N) for j in range(NU) if act[i, j] != FREE}
    ox, ou, op = 0, NX * (N + 1), NX * (N + 1) + len(free)       # offsets of dx, du_free, pi (pi_{-1} first)
    n = op + NX * (N + 1)
    M, rhs = mp.zeros(n, n), mp.zeros(n, 1)
    row = 0
    for c in range(NX):                                            # dx_0 = d0
        M[row, ox + c] = 1; rhs[row] = qp.d0[c]; row += 1
    for i in range(N):                                             # dx_{i+1} - A dx_i - B du = b
        for c in range(NX):
            M[row, ox + NX * (i + 1) + c] = 1
            rhs[row] = qp.b[i][c]
            for k in range(NX):
                M[row, ox + NX * i + k] -= qp.A[i][c][k]
            for j in range(NU):
                if (i, j) in held:
                    rhs[row] += qp.B[i][c][j] * held[(i, j)]
                else:
                    M[row, ou + free.index((i, j))] -= qp.B[i][c][j]
            row += 1
    for i in range(N + 1):                                         # Qd dx_i + q_i + A_i' pi_i - pi_{i-1} = 0
        for c in range(NX):
            M[row, ox + NX * i + c] = qp.Qd[i][c]
            rhs[row] = -qp.q[i][c]
            M[row, op + NX * i + c] -= 1                           # pi_{i-1} sits at block i
            if i < N:
                for k in range(NX):
                    M[row, op + NX * (i + 1) + k] += qp.A[i][k][c]
            row += 1
    for f, (i, j) in enumerate(free):                              # Rd du + r + B' pi_i = 0
        M[row, ou + f] = qp.Rd[i][j]
        rhs[row] = -qp.r[i][j]
        for k in range(NX):
            M[row, op + NX * (i + 1) + k] += qp.B[i][k][j]
        row += 1
    assert row == n
    z = mp.lu_solve(M, rhs)
    dx = [[z[ox + NX * i + c] for c in range(NX)] for i in range(N + 1)]
    du = [[held[(i, j)] if (i, j) in held else z[ou + free.index((i, j))] for j in range(NU)] for i in range(N)]
    pi = [[z[op + NX * (i + 1) + c] for c in range(NX)] for i in range(N)]
    g = [[qp.Rd[i][j] * du[i][j] + qp.r[i][j] + sum((qp.B[i][k][j] * pi[i][k] for k in range(NX)), zero) for j in range(NU)] for i in range(N)]
    return dict(dx=dx, du=du, pi=pi, g=g)


@pytest.mark.parametrize("N,seed", [(2, 1), (3, 2)])
def test_solve_on_equals_a_dense_kkt_solve(N, seed):
    K = MpBackend()
    rng = np.random.default_rng(seed)
    qp = _random_qp(K, N, rng)
    act = rng.choice([LOWER, FREE, FREE, UPPER], size=(N, NU))
    act[0, 0], act[N - 1, 1], act[0, 2] = LOWER, UPPER, FREE
    with K.mp.workdps(90):       # the dense elimination loses digits the structured one does not: it runs with more
        ref = _dense_solve(qp, act)
    got = qp.solve_on(act)
    tol, worst = K.lit("1e-50"), K.lit("0")
    for name in ("dx", "du", "pi", "g"):
        for a, e in zip(got[name], ref[name]):
            for x, y in zip(a, e):
                worst = max(worst, abs(x - y) / max(1, abs(y)))
    print(f"[qp_exact] solve_on against the dense KKT solve at N = {N}: {float(worst):.1e}")
    assert worst <= tol
    for i in range(N):           # multipliers: the gradient on the held inputs, with the bound's sign
        for j in range(NU):
            assert got["lam"][i][j] == (got["g"][i][j] if act[i, j] == LOWER else 0) and got["lam"][i][NU + j] == (-got["g"][i][j] if act[i, j] == UPPER else 0)


@pytest.fixture(scope="module")
def tight_case(oracle):
    """row 0 (N = 4), kind c, tick 1: the QP, its certified set and minimiser"""
    r, kind = 0, "c"
    row = C.ROWS[r]
    o, W, We, ts, W0, lbu, ubu = C.oracle_options(oracle, row, kind)
    ins = C.instance(r, kind, C.seeds_of(r, kind)[0])
    A, B, b = C.oracle_linearisation(oracle, ins["x"], ins["u"], ins["p"], ts, ins["rp"])
    from qp_exact import build_qp
    qp = build_qp(ins["x"], ins["u"], ins["x0"], ins["yrefs"][0], W, We, ts, lbu, ubu, A, B, b, W0=W0)
    pi, lam = np.zeros((row.N, NX)), np.zeros((row.N, 8))
    ot = C.oracle_tick(oracle, o, A, B, b, ins["x"], ins["u"], pi, lam, ins["x0"], ins["yrefs"][0], W, We, ts, lbu, ubu, W0)
    sol, act, margins, rounds = qp.minimiser(ot["act"])
    assert rounds == 0 and (act != FREE).sum() >= 3 and (act == FREE).any()
    return qp, sol, act, margins


def test_certify_rejects_a_wrong_active_set(tight_case):
    qp, sol, act, margins = tight_case
    assert qp.certify(sol, act) == margins and min(margins) > C.MARGIN
    i, j = np.argwhere(act == FREE)[0]
    more = act.copy(); more[i, j] = LOWER                   # one bound too many: its multiplier has the wrong sign
    with pytest.raises(NotCertified) as e:
        qp.certify(qp.solve_on(more), more)
    assert e.value.bad_mult is not None and e.value.bad_mult[2] < 0
    i, j = np.argwhere(act != FREE)[0]
    fewer = act.copy(); fewer[i, j] = FREE                  # one too few: the released input leaves its box
    with pytest.raises(NotCertified) as e:
        qp.certify(qp.solve_on(fewer), fewer)
    assert e.value.kind == "bound" and e.value.bad_bound[2] < 0
    with pytest.raises(NotCertified) as e:                  # a solution of ANOTHER set does not satisfy this set's equations
        qp.certify(qp.solve_on(more), act)
    assert e.value.kind == "residual"


def test_repair_loop_from_the_empty_guess(tight_case):
    qp, sol, act, margins = tight_case
    sol2, act2, margins2, rounds = qp.minimiser(np.full(act.shape, FREE))
    print(f"[qp_exact] repair from the empty guess: {rounds} rounds to {int((act2 != FREE).sum())} active bounds")
    assert 0 < rounds <= 8 * qp.N and np.array_equal(act2, act) and margins2 == margins
    assert all(a == b for x, y in zip(sol2["du"], sol["du"]) for a, b in zip(x, y))
    with pytest.raises(NotCertified):
        qp.minimiser(np.full(act.shape, FREE), max_rounds=1)


# ---- 2. the oracle against the certified minimiser, every case ---------------------------------------------------------------------------
def test_case_table_is_complete():
    for r, row in enumerate(C.ROWS):
        for kind in ("a", "c", "d"):
            assert len(C.SEEDS[(r, kind)]) == row.B, (r, kind)
        assert row.B <= (1 if row.N > 80 else 2 if row.N > 40 else 4)


@pytest.mark.parametrize("r", range(len(C.ROWS)), ids=[C.row_name(row) for row in C.ROWS])
def test_oracle_against_the_certified_minimiser(oracle, pool, r):
    row = C.ROWS[r]
    todo = [(r, kind, seed) for kind in C.KINDS for seed in C.seeds_of(r, kind)]
    results = list(pool.map(C.cpu_case_job, todo))           # (a failed condition of a case is raised here: no case is left out)
    worst = {}
    for (_, kind, seed), ticks in zip(todo, results):
        assert len(ticks) == C.TICKS
        for k, t in enumerate(ticks):
            print(f"[qp_exact] {C.row_name(row)} kind {kind} seed {seed} tick {k + 1}: slack {t['slack']:.2e} multiplier {t['mult']:.2e} "
                  f"active {t['n_act']} repair rounds {t['rounds']} oracle Newton systems {t['iters']}")
            assert (t["iters"] == 0) == (kind == "a"), (kind, seed, k, t["iters"])
            for q, e in t["err"].items():
                worst[q] = max(worst.get(q, 0.0), e)
    print(f"[qp_exact] {C.row_name(row)}: oracle scaled errors " + ", ".join(f"{q} {e:.1e}" for q, e in worst.items()))
    assert 4.0 * max(worst.values()) < ORACLE_CEILING, worst
    if row.extra != "dist6":
        # the data is orc_rti_step's own: its dumped linearisation is the one used above, bit for bit, and its records meet the exact ones
        kind, seed = "c", C.seeds_of(r, "c")[0]
        o, W, We, ts, W0, lbu, ubu = C.oracle_options(oracle, row, kind)
        ins = C.instance(r, kind, seed)
        x, u, pi, lam = ins["x"].copy(), ins["u"].copy(), np.zeros((row.N, NX)), np.zeros((row.N, 8))
        A, B, b = C.oracle_linearisation(oracle, x, u, ins["p"], ts, None)
        out = oracle.rti_step(o, ins["x0"], ins["yrefs"][0], ins["p"], x, u, pi, lam, want_lin=True)
        assert out["status"] == 0 and np.array_equal(out["A"], A) and np.array_equal(out["B"], B) and np.array_equal(out["b"], b)
        ex = results[todo.index((r, kind, seed))][0]
        assert C.scaled_err(x, ex["x"]).max() * 4.0 < ORACLE_CEILING and C.scaled_err(u, ex["u"]).max() * 4.0 < ORACLE_CEILING
        assert np.abs(out["u0"] - ex["u"][0]).max() < 1e-9


# ---- 3. the independent recipe --------------------------------------------------------------------------------------------------------------
def test_bvls_recipe_against_the_certified_minimiser(oracle):
    import oracle.oracle_ffi as F
    F.build()
    if not os.path.exists(F.REF_SO):
        pytest.skip("oracle/_ref (the reference's CasADi C, built where the reference tree is present) is not here")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import make_golden as G
    r, kind = 2, "c"
    row = C.ROWS[r]
    assert row.N == 20
    o, W, We, ts, W0, lbu, ubu = C.oracle_options(oracle, row, kind)
    seed = C.seeds_of(r, kind)[0]
    ins = C.instance(r, kind, seed)
    ex = C.cpu_case(oracle, r, kind, seed, exact_tick, ticks=1)[0]["ex"]
    xb, ub, info = G.rti_step_independent(F.CasadiRef(), row.N, row.Ts, ins["x0"], ins["yrefs"][0], ins["p"], ins["x"], ins["u"], Wd=W, lbu=lbu,
                                          ubu=ubu, Wed=We)
    e = float(np.abs(ub - ex["u"]).max())
    print(f"[qp_exact] BVLS recipe at N = 20, {info['nact']} active bounds: |u - u_exact| {e:.1e}, |x - x_exact| {float(np.abs(xb - ex['x']).max()):.1e}")
    assert info["nact"] == int((ex["act"] != FREE).sum()) and info["qp_kkt"] < 1e-9
    assert e < 1e-9
