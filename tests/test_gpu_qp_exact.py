"""The QP layer of every kernel family -- Riccati factorisation, active-set rounds, interior-point loop, final active-set solve, the
multipliers and the records -- against the certified 60-digit minimiser of the SAME QP (tests/qp_exact.py), entry by entry.

Every row of tests/qp_exact_cases.py (one kernel instantiation each) runs its four kinds of instance for two ticks.  Per (row, kind) two
solvers take the same inputs: one with debug_dump_linearisation(True), whose A, B, b are the QP's data, and one as the product runs (no
dump: at the resident windowed horizons the parallel-in-time kernel goes first, and pit_last() says who completed each instance).  The QP
is formed in exact arithmetic from the device's own linearisation, its minimiser certified from the active set oracle.qp_solve finds on
the same data (never from the device's answer), and BOTH solvers' new iterates, multipliers and records are compared with it.  Tick 2
enters from tick 1's exact minimiser (rounded to double) on both sides.

The bar is tests/test_gpu_model_exact.py's: scaled error |got - ref| / max(1, |ref|) <= 4 x max(E_orc, 2^-50) per (row, kind) and quantity,
E_orc = the worst error of oracle.qp_solve on the same device-dumped data against the same minimiser (its step taken as orc_rti_step takes
it, x + dx, and the difference to the entering iterate formed as the device's is; cost and KKT residual by the oracle's formulas in double),
never an error measured on the device.  The factor: other summation order, FMAs, Newton reciprocals -- each the size of the oracle's own
rounding.  u0 is also held to 1e-9 absolute.  ONE widening: an instance that misses the plain bar may add D = N x the largest scaled
change of the quantity when every entry of A, B, b, q, r, d0 is multiplied by 1 + s 2^-53 (s = +-1, three seeded draws) and the QP is solved
again, exactly, on its certified set: the first-order effect of rounding the data once per stage.  The share of D used stands beside the
figure.  No case is excused, dropped or skipped.

The figures are printed (pytest -s) and, with BROV_QP_EXACT_REPORT=<file> set, written there (profiles/qp_exact.txt is a copy)."""
import concurrent.futures
import multiprocessing
import os

import numpy as np
import pytest

import qp_exact_cases as C
from qp_exact import NX, QUANTITIES, exact_tick

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2.0 ** -50
U0_ABS = 1e-9
PERTURB_SEEDS = (1, 2, 3)
_MEASURED = {}


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


@pytest.fixture(scope="module")
def pool():
    # spawn, not fork: the parent holds a HIP context
    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    p = concurrent.futures.ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn"))
    yield p
    p.shutdown()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("BROV_QP_EXACT_REPORT")
    if not _MEASURED or not path:
        return
    with open(path, "w") as f:
        f.write("device QP layer against the certified 60-digit minimiser (tests/test_gpu_qp_exact.py)\n"
                "per quantity: worst device scaled error (oracle's on the same data, ratio = device / max(oracle, 2^-50)); the bar is 4\n"
                "dump: the solver whose linearisation is read back; plain: the product's launch\n\n")
        for k in _MEASURED:
            f.write(f"{k}: {_MEASURED[k]}\n")


def _note(key, text):
    _MEASURED[key] = text
    print(f"[qp_exact] {key}: {text}")


def _solver(ba, row, kind, B, lbu, ubu, ts, W0, rp, dump):
    os.environ.update(row.env)
    try:
        s = ba.BatchSolver(B, ba.SolverOptions(row.N, row.Ts, kernel_path=row.path, lbu=list(lbu), ubu=list(ubu), qp_early_exit=0 if kind == "b" else 1))
    finally:
        for k in row.env:
            os.environ.pop(k, None)
    if row.extra == "grid":
        s.set_time_steps(ts); s.set_stage0_weight(W0)
    if row.extra == "dist6":
        s.enable_dist6(); s.set_rp_disturbance(rp)
    s.debug_dump_linearisation(dump)
    return s


def _kernel_checks(ba, s, row):
    """the kernel that served the solve is the row's; returns its name for the record"""
    info = s.lds_kernel_info()
    if row.path == 1:
        assert s.last_kernel_path() == ba.PATH_STREAMING
        return "streaming pair"
    if row.win is None:
        assert s.last_kernel_path() == ba.PATH_FUSED and (info["kind"].startswith("fused") if row.kind == "fused*" else info["kind"] == row.kind), info
        return info["kind"]
    assert s.last_kernel_path() == ba.PATH_WINDOWED and info["kind"] == row.kind and s.window_stages() == row.win, (info, s.window_stages())
    assert info["threads_per_block"] == (256 if row.kind.endswith("resident") else 64), info
    return f"{info['kind']}, {s.window_stages()} stages per window" + (", rti_window_kernel_long" if row.N > 128 else "")


def _answer(s, x, u):
    """what a solver left: dict(dx, du: new iterate minus the entering one; pi, lam, u0, cost, kkt [B...]) and its records"""
    res = s.results()
    gx, gu, gpi, glam = s.get_iterate()
    return dict(dx=gx - x, du=gu - u, pi=gpi, lam=glam, u0=res["u0"], cost=res["cost"], kkt=res["kkt"]), res


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("r", range(len(C.ROWS)), ids=[C.row_name(row).replace(" ", "_") for row in C.ROWS])
def test_qp_layer_against_the_certified_minimiser(ba, oracle, pool, r, kind):
    row = C.ROWS[r]
    N, B = row.N, row.B
    o, W, We, ts, W0, lbu, ubu = C.oracle_options(oracle, row, kind)
    ins = [C.instance(r, kind, seed) for seed in C.seeds_of(r, kind)]
    assert len(ins) == B
    x, u = np.stack([i["x"] for i in ins]), np.stack([i["u"] for i in ins])
    pi, lam = np.zeros((B, N, NX)), np.zeros((B, N, 8))
    x0, p = np.stack([i["x0"] for i in ins]), np.stack([i["p"] for i in ins])
    rp = np.stack([i["rp"] for i in ins]) if row.extra == "dist6" else None
    solvers = {"dump": _solver(ba, row, kind, B, lbu, ubu, ts, W0, rp, True), "plain": _solver(ba, row, kind, B, lbu, ubu, ts, W0, rp, False)}
    assert np.array_equal(solvers["dump"].opts.W, W) and np.array_equal(solvers["dump"].opts.We, We)
    what = f"{C.row_name(row)} kind {kind}"
    dev = {k: {q: [] for q in QUANTITIES} for k in solvers}      # scaled errors per solver and quantity: [tick][instance] arrays of entries
    orc = {q: [] for q in QUANTITIES}
    refs, served, pit, margins, u0_abs = [], "", [], [], 0.0
    for k in range(C.TICKS):
        yref = np.stack([i["yrefs"][k] for i in ins])
        got = {}
        for name, s in solvers.items():
            s.set_iterate(x=x, u=u, pi=pi, lam=lam)
            s.set_x0(x0); s.set_params(p); s.set_yref(yref)
            s.solve(sync=True)
            got[name], res = _answer(s, x, u)
            assert np.all(res["status"] == 0), (what, name, k, res["status"])
            served = _kernel_checks(ba, s, row)
            if kind == "a":
                assert np.all(res["qp_iter"] == 0), (what, name, k, res["qp_iter"])
            if kind == "b":
                assert np.all(res["qp_iter"] > 0), (what, name, k, res["qp_iter"])
        if row.kind == "windowed, resident":
            pit.append(solvers["plain"].pit_last().tolist())
            assert not solvers["dump"].pit_last().any()
        A, Bm, bv = solvers["dump"].linearisation()
        ot = [C.oracle_tick(oracle, o, A[b], Bm[b], bv[b], x[b], u[b], pi[b], lam[b], x0[b], yref[b], W, We, ts, lbu, ubu, W0) for b in range(B)]
        assert all(t["status"] == 0 for t in ot), (what, k, [t["status"] for t in ot])
        jobs = [C.job_of(x[b], u[b], pi[b], lam[b], x0[b], yref[b], W, We, W0, ts, lbu, ubu, A[b], Bm[b], bv[b], ot[b]["act"]) for b in range(B)]
        ex = list(pool.map(exact_tick, jobs))
        for b in range(B):
            C.hold_kind(row, kind, k, ex[b], lbu[None] - u[b], ubu[None] - u[b], early=ot[b]["early"] if kind == "a" else None)
            margins.append((ex[b]["slack"], ex[b]["mult"], int((ex[b]["act"] != 0).sum())))
            for q in QUANTITIES:
                orc[q].append(C.scaled_err(ot[b][q], ex[b][q]))
                for name in solvers:
                    dev[name][q].append(C.scaled_err(got[name][q][b], ex[b][q]))
            for name in solvers:
                u0_abs = max(u0_abs, float(np.abs(got[name]["u0"][b] - ex[b]["u0"]).max()))
        refs.append((jobs, ex))
        x, u = np.stack([e["x"] for e in ex]), np.stack([e["u"] for e in ex])
        pi, lam = np.stack([e["pi"] for e in ex]), np.stack([e["lam"] for e in ex])
    for s in solvers.values():
        s.close()

    # ---- the bar, per quantity; an instance over it may add D, computed from the exact solver and its own data alone
    parts, bad = [], []
    widened = {}
    for q in QUANTITIES:
        e_orc = max(float(np.max(v)) for v in orc[q])
        bar = FACTOR * max(e_orc, FLOOR)
        for name in solvers:
            worst = max(float(np.max(v)) for v in dev[name][q])
            text = f"{name} {q} {worst:.2e} (oracle {e_orc:.2e}, ratio {worst / (bar / FACTOR):.2f}"
            over = [j for j, v in enumerate(dev[name][q]) if not np.all(v <= bar)]      # (a NaN is over)
            used = 0.0
            for j in over:
                k, b = divmod(j, B)
                if (k, b) not in widened:
                    jobs, _ = refs[k]
                    widened[(k, b)] = exact_tick(dict(jobs[b], perturb=PERTURB_SEEDS))["D"]
                D = N * widened[(k, b)][q]
                v = dev[name][q][j]
                if not np.all(v <= bar + D):
                    bad.append((name, q, f"tick {k + 1} instance {b}", float(np.max(v)), bar, D))
                used = max(used, float(np.max(v) - bar) / D if D > 0 else np.inf)
            if over:
                text += (f"; {len(over)} of {len(dev[name][q])} instance-ticks over the plain bar: the data rounded once per stage moves this quantity by "
                         f"D, of which at most {used:.3f} is used")
            parts.append(text + ")")
    _note(what, f"{served}; margins (slack, multiplier, active bounds) per tick and instance {[(f'{a:.1e}', f'{m:.1e}', n) for a, m, n in margins]}"
          + (f"; completed by rti_pit_kernel (plain, per tick) {pit}" if pit else "") + f"; |u0 - exact| {u0_abs:.1e}; " + "; ".join(parts))
    assert not bad, (what, bad)
    assert u0_abs <= U0_ABS, (what, u0_abs)
