"""The device model, its ERK4 step in every copy and its sensitivity columns in every kernel family against a 60-digit reference
(tests/model_exact.py; fixture tests/golden/model_exact.npz, scripts/make_model_exact_golden.py), entry by entry.

The bar.  Errors are scaled |got - ref| / max(1, |ref|) per entry.  sincos_pio2 and rcp_nr, through the test hook
(csrc/model_selftest.hip), are held in units of the last place: 2 ulp for |a| <= 1e6 (a host run of the same IEEE operations gives 1.53)
and 1 ulp.  Everything else: scaled error <= 4 x max(E_orc, 2^-50), E_orc = the worst error of the double-precision oracle on the same
family and quantity against the SAME reference (stored with the fixture; computed here for inputs that exist only at run time), never
an error measured on the device.  The factor 4: the device's trig is good to 1.5 ulp where libm's is to 0.5, its reciprocals are Newton
steps, and its sums are contracted into FMAs in another order -- each of the size of the oracle's own rounding.  No case is excused.

Run-time inputs (the plants: the input is what the solver computed): every step the device took is compared, with the oracle's error
at the same inputs as E_orc.  Four families (WIDER: kinks, far yaw, steep pitch, small masses) may add, on a step that misses, a
first-order bound of what rounding the state does, computed with the exact model: the cause and the bound stand beside the figures.
The one-launch loop, which diverges from these states, has its own paragraph in its test.

The figures of a run are printed (pytest -s) and, with BROV_MODEL_EXACT_REPORT=<file> set, written there (profiles/model_exact.txt is a copy)."""
import math
import os

import numpy as np
import pytest

from model_exact import ExactModel, backend, scaled_err
from wrench_restatement import f_under_wrench, rk4_under_wrench

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR, FLOOR = 4.0, 2.0 ** -50
S_MAX = 50.0          # scripts/make_model_exact_golden.py
QF, QX, QS = 0, 1, 2  # columns of E_orc: f, x+, S
_MEASURED = {}


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


@pytest.fixture(scope="module")
def fx():
    g = np.load(os.path.join(ROOT, "tests", "golden", "model_exact.npz"))
    d = {k: g[k] for k in g.files}
    d["names"] = list(d["families"])
    return d


@pytest.fixture(scope="module")
def exact():
    """mpmath at 60 digits; numpy.longdouble with a 64-bit mantissa where mpmath is missing; else the tests fail"""
    return ExactModel(backend())


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("BROV_MODEL_EXACT_REPORT")
    if not _MEASURED or not path:
        return
    with open(path, "w") as f:
        f.write("device model against the 60-digit reference (tests/test_gpu_model_exact.py)\n"
                "ratio = worst device scaled error / max(worst oracle scaled error, 2^-50); the bar is 4\n\n")
        for k in sorted(_MEASURED):
            f.write(f"{k}: {_MEASURED[k]}\n")


def _note(key, text):
    _MEASURED[key] = text
    print(f"[model_exact] {key}: {text}")


def _hold(what, fam, dev_err, orc_worst, names):
    """dev_err [cases]: the device's worst scaled error per case; fam [cases]; orc_worst [families]: E_orc of the quantity.  Every case
    of every family within FACTOR x max(E_orc, FLOOR); the ratios are recorded first."""
    dev_err, fam = np.asarray(dev_err), np.asarray(fam)
    parts, bad = [], []
    for fi in np.unique(fam):
        bar = FACTOR * max(float(orc_worst[fi]), FLOOR)
        worst = float(np.max(dev_err[fam == fi]))
        parts.append(f"{names[fi]} {worst:.2e} (oracle {float(orc_worst[fi]):.2e}, ratio {worst / (bar / FACTOR):.2f})")
        if not np.all(dev_err[fam == fi] <= bar):      # (a NaN fails)
            bad.append((names[fi], worst, bar))
    _note(what, "; ".join(parts))
    assert not bad, (what, bad)


def _family_worst(err, fam, nfam):
    return np.array([np.max(err[fam == fi]) if np.any(fam == fi) else 0.0 for fi in range(nfam)])


# ---- 1. sincos_pio2 and rcp_nr in units of the last place --------------------------------------------------------------------------------
def _trig_arguments():
    import mpmath
    mp = mpmath.mp.clone(); mp.dps = 50
    rng = np.random.default_rng(7)
    ks = np.concatenate([np.arange(-2000, 2001), rng.integers(-640000, 640001, 4000)])
    on = np.array([float(mp.pi * int(k) / 2) for k in ks])
    kh = np.arange(-2000, 2001)
    half = np.array([float(mp.pi * (2 * int(k) + 1) / 4) for k in kh])
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 2.2250738585072014e-308, 1e-200, -1e-100, 1e-30, 1e-17, -1e-9, 1e-8, 3e-5])
    a = np.concatenate([on, np.nextafter(on, np.inf), np.nextafter(on, -np.inf), half, np.nextafter(half, np.inf),
                        rng.uniform(-1e6, 1e6, 20000), rng.uniform(-400, 400, 20000), tiny])
    return mp, a


def _ulps(got, hi, lo):
    """|got - (hi + lo)| / ulp(hi), hi = the double nearest to the exact value, lo = the rest (got - hi is exact where it matters)"""
    ulp = np.array([math.ulp(v) for v in hi])
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs((got - hi) - lo) / ulp
    return np.where((hi == 0.0) & (got == 0.0), 0.0, e)


def test_sincos_and_reciprocal_in_ulps(ba):
    from bluerov2_amd.solver import selftest_model
    mp, a = _trig_arguments()
    assert np.abs(a).max() <= 640000 * 1.5707963267948968 + 1 and len(a) > 70000
    special = np.array([np.inf, -np.inf, np.nan])
    # d from 1 to 100: every integer, powers of two and their neighbours, a uniform sample
    rng = np.random.default_rng(8)
    d = np.concatenate([np.arange(1.0, 101.0), np.nextafter(2.0 ** np.arange(0, 7), 0.0)[1:], np.nextafter(2.0 ** np.arange(0, 7), np.inf)[:-1],
                        rng.uniform(1.0, 100.0, 4000)])
    n = len(a) + len(special)
    dd = np.ones(n); dd[:len(d)] = d
    out = selftest_model(a=np.concatenate([a, special]), d=dd)
    assert np.isnan(out["sin"][-3:]).all() and np.isnan(out["cos"][-3:]).all()      # +-Inf and NaN give NaN
    sn, cs = out["sin"][:len(a)], out["cos"][:len(a)]
    hi, lo = np.empty((2, len(a))), np.empty((2, len(a)))
    for i, v in enumerate(a):
        c, s = mp.cos_sin(mp.mpf(float(v)))
        hi[0, i] = float(s); lo[0, i] = float(s - mp.mpf(hi[0, i]))
        hi[1, i] = float(c); lo[1, i] = float(c - mp.mpf(hi[1, i]))
    es, ec = _ulps(sn, hi[0], lo[0]), _ulps(cs, hi[1], lo[1])
    quadrant = int(np.sum(np.abs(sn - hi[0]) > 0.5) + np.sum(np.abs(cs - hi[1]) > 0.5))
    i_s, i_c = int(np.argmax(es)), int(np.argmax(ec))
    _note("1 sincos_pio2", f"worst sin {es[i_s]:.3f} ulp at a = {a[i_s]!r}, worst cos {ec[i_c]:.3f} ulp at a = {a[i_c]!r}, over {len(a)} arguments "
          f"|a| <= 1e6; quadrant errors {quadrant}; sin(-0.0) = {sn[np.nonzero((a == 0) & np.signbit(a))[0][0]]!r}")
    rq = out["rcp"][:len(d)]
    rh = np.array([float(1 / mp.mpf(float(v))) for v in d])
    rl = np.array([float(1 / mp.mpf(float(v)) - mp.mpf(float(h))) for v, h in zip(d, rh)])
    er = _ulps(rq, rh, rl)
    _note("1 rcp_nr", f"worst {er.max():.3f} ulp of 1/d at d = {d[int(np.argmax(er))]!r}, over {len(d)} values of d in [1, 100]; "
          f"correctly rounded in {int(np.sum(rq == rh))}")
    assert quadrant == 0
    assert es.max() <= 2.0 and ec.max() <= 2.0, (es.max(), a[i_s], ec.max(), a[i_c])
    assert er.max() <= 1.0, (er.max(), d[int(np.argmax(er))])


# ---- 2. model_f, both instantiations, row by row -------------------------------------------------------------------------------------------
def test_model_f_both_instantiations_on_every_family(ba, oracle, exact, fx):
    from bluerov2_amd.solver import selftest_model
    names, fam = fx["names"], fx["family"]
    wf = names.index("world_wrench")
    out = selftest_model(x=fx["x"], u=fx["u"], p=fx["p"], ww=fx["ww"], rp=fx["rp"])
    # with the world wrench (zero outside its family, where the projection then adds zeros): the fixture's f
    _hold("2 model_f<WorldWrench>", fam, scaled_err(out["f_ww"], fx["f"]).max(axis=1), fx["E_orc"][:, QF], names)
    # without: the fixture's f outside the world-wrench family; there, the exact model and the oracle without the wrench, here
    ref, orc = fx["f"].copy(), fx["E_orc"][:, QF].copy()
    w_idx = np.nonzero(fam == wf)[0]
    for c in w_idx:
        ref[c] = exact.f_double(fx["x"][c], fx["u"][c], fx["p"][c])
    orc[wf] = max(scaled_err(oracle.f(fx["x"][c], fx["u"][c], fx["p"][c]), ref[c]).max() for c in w_idx)
    _hold("2 model_f<NoWorldWrench>", fam, scaled_err(out["f"], ref).max(axis=1), orc, names)
    assert np.abs(out["f"][w_idx] - out["f_ww"][w_idx]).max() > 1.0        # the wrench is felt


# ---- 3. the linearisation of every kernel family ---------------------------------------------------------------------------------------------
def _in_turn(fam, idx):
    """idx reordered so that the families take turns: first case of each, second case of each, ..."""
    rank = np.array([np.sum(fam[idx[:j]] == fam[idx[j]]) for j in range(len(idx))])
    return idx[np.lexsort((fam[idx], rank))]


def _cells(fx, h, B, N, dist6):
    """fixture cases of step h for the (N + 1) nodes of B instances, the families taking turns"""
    names, fam = fx["names"], fx["family"]
    ok = (fx["h"] == h) & (fam != names.index("world_wrench"))
    if not dist6:
        ok &= fam != names.index("dist6")
    idx = _in_turn(fam, np.nonzero(ok)[0])
    assert len(idx) >= 20 and len(np.unique(fam[idx])) == (7 if dist6 else 6)
    return idx[np.arange(B * (N + 1)) % len(idx)].reshape(B, N + 1)


def _check_linearisation(s, fx, cell, ref_xn, ref_S, orc_x, orc_S, what):
    """A, B, b of every instance and stage against the exact x+ and S of the cells; b = x+ - x_{k+1} as the oracle's want_lin gives it"""
    names, fam = fx["names"], fx["family"]
    B, N = cell.shape[0], cell.shape[1] - 1
    x = fx["x"][cell]
    A, Bm, bb = s.linearisation()
    S = np.concatenate([A, Bm], axis=-1)                                   # [B, N, 12, 16]
    assert np.array_equal(S[..., :3], np.broadcast_to(np.eye(12)[:, :3], (B, N, 12, 3))), what       # position columns: the identity block
    eS = scaled_err(S, ref_S).reshape(B * N, -1).max(axis=1)
    b_ref = ref_xn - x[:, 1:]
    scale = np.maximum(1.0, np.maximum(np.abs(ref_xn), np.abs(x[:, 1:])))
    eb = (np.abs(bb - b_ref) / scale).reshape(B * N, -1).max(axis=1)
    f = fam[cell[:, :N]].reshape(-1)
    _hold(f"3 {what} S", f, eS, orc_S, names)
    _hold(f"3 {what} b", f, eb, orc_x, names)


LIN = [   # N, Ts, path, B, environment, kind of the LDS kernel, stages per window (None: not a windowed kernel)
    (4, 0.05, 1, 12, {}, None, None), (4, 0.05, 2, 12, {}, "fused*", None),
    (10, 0.1, 1, 5, {}, None, None), (10, 0.1, 2, 5, {}, "fused, two waves per SIMD", None),
    (20, 0.05, 1, 3, {}, None, None), (20, 0.05, 2, 3, {}, "fused", None),
    (40, 0.0125, 1, 2, {}, None, None),
    (40, 0.0125, 2, 2, {}, "windowed, resident", 40),                                   # four waves, a quarter of the horizon each
    (40, 0.0125, 2, 3, {"BROV_DEV_WIN_BLOCKS": "1"}, "windowed, resident", 40),       # ... and wave 0 alone in sub-chunks for the block's next instances
    (40, 0.0125, 2, 2, {"BROV_DEV_NO_RESIDENT": "1"}, "windowed", 20),                # windows of 20 stages
    (80, 0.0125, 2, 2, {}, "windowed, resident", 80),                                   # B <= 4 at N = 80: four waves x 20 intervals
]


@pytest.mark.parametrize("N,Ts,path,B,env,kind,win", LIN)
def test_linearisation_on_fixture_points(ba, fx, N, Ts, path, B, env, kind, win):
    os.environ.update(env)
    try:
        s = ba.BatchSolver(B, ba.SolverOptions(N, Ts, kernel_path=path))
    finally:
        for k in env:
            os.environ.pop(k, None)
    cell = _cells(fx, Ts, B, N, dist6=False)
    s.set_iterate(x=fx["x"][cell], u=fx["u"][cell[:, :N]], pi=np.zeros((B, N, 12)), lam=np.zeros((B, N, 8)))
    s.set_x0(fx["x"][cell[:, 0]]); s.set_params(fx["p"][cell]); s.set_yref(np.zeros((N + 1, 16)))
    s.debug_dump_linearisation(True)
    s.solve(sync=True)
    info = s.lds_kernel_info()
    if path == 1:
        assert s.last_kernel_path() == ba.PATH_STREAMING
    elif win is None:
        assert s.last_kernel_path() == ba.PATH_FUSED and (info["kind"].startswith("fused") if kind == "fused*" else info["kind"] == kind), info
    else:
        assert s.last_kernel_path() == ba.PATH_WINDOWED and info["kind"] == kind and (s.window_stages() == win or 0 < s.window_stages() <= win < N), (info, s.window_stages())
        assert info["threads_per_block"] == (256 if kind.endswith("resident") else 64), info
    what = f"N={N} path={path} B={B} {kind or 'streaming'}" + (" " + ",".join(env) if env else "")
    _check_linearisation(s, fx, cell, fx["xn"][cell[:, :N]], fx["S"][cell[:, :N]], fx["E_orc"][:, QX], fx["E_orc"][:, QS], what)
    s.close()


@pytest.mark.parametrize("path", [1, 2])
def test_linearisation_with_the_two_moments(ba, fx, path):
    N, Ts, B = 20, 0.05, 3
    s = ba.BatchSolver(B, ba.SolverOptions(N, Ts, kernel_path=path))
    s.enable_dist6()
    cell = _cells(fx, Ts, B, N, dist6=True)
    assert (fx["family"][cell] == fx["names"].index("dist6")).sum() >= 6
    s.set_iterate(x=fx["x"][cell], u=fx["u"][cell[:, :N]], pi=np.zeros((B, N, 12)), lam=np.zeros((B, N, 8)))
    s.set_x0(fx["x"][cell[:, 0]]); s.set_params(fx["p"][cell]); s.set_rp_disturbance(fx["rp"][cell]); s.set_yref(np.zeros((N + 1, 16)))
    s.debug_dump_linearisation(True)
    s.solve(sync=True)
    assert s.last_kernel_path() == path
    _check_linearisation(s, fx, cell, fx["xn"][cell[:, :N]], fx["S"][cell[:, :N]], fx["E_orc"][:, QX], fx["E_orc"][:, QS], f"dist6 N=20 path={path}")
    s.close()


@pytest.mark.parametrize("path", [1, 2])
def test_linearisation_on_a_geometric_grid(ba, oracle, exact, fx, path):
    """steps from 0.0125 to 0.1 in a geometric progression: none but the ends is a step of the fixture, so the reference and the oracle's
    error are computed here, at one instance.  A case is used at steps up to the one the fixture keeps it at (well conditioned there)."""
    assert exact.K.name == "mpmath", "the sensitivities of run-time inputs need mpmath"
    N, B = 20, 1
    names, fam = fx["names"], fx["family"]
    ts = 0.0125 * 8.0 ** (np.arange(N) / (N - 1.0))
    usable = (fam != names.index("world_wrench")) & (fam != names.index("dist6"))
    cell = np.empty((B, N + 1), dtype=int)
    for k in range(N + 1):
        idx = _in_turn(fam, np.nonzero(usable & (fx["h"] >= min(ts[min(k, N - 1)], 0.1)))[0])
        cell[0, k] = idx[k % len(idx)]
    assert len(np.unique(fam[cell])) == 6
    s = ba.BatchSolver(B, ba.SolverOptions(N, float(ts[0]), kernel_path=path))
    s.set_time_steps(ts)
    s.set_iterate(x=fx["x"][cell], u=fx["u"][cell[:, :N]], pi=np.zeros((B, N, 12)), lam=np.zeros((B, N, 8)))
    s.set_x0(fx["x"][cell[:, 0]]); s.set_params(fx["p"][cell]); s.set_yref(np.zeros((N + 1, 16)))
    s.debug_dump_linearisation(True)
    s.solve(sync=True)
    assert s.last_kernel_path() == path
    xn, S, ex, eS = np.empty((B, N, 12)), np.empty((B, N, 12, 16)), np.zeros(N), np.zeros(N)
    for k in range(N):
        c = cell[0, k]
        xn[0, k], S[0, k] = exact.sens(fx["x"][c], fx["u"][c], fx["p"][c], float(ts[k]))
        oxn, oA, oB = oracle.rk4_sens(fx["x"][c], fx["u"][c], fx["p"][c], float(ts[k]))
        ex[k], eS[k] = scaled_err(oxn, xn[0, k]).max(), scaled_err(np.concatenate([oA, oB], axis=1), S[0, k]).max()
        assert np.abs(S[0, k]).max() <= S_MAX
    f = fam[cell[0, :N]]
    _check_linearisation(s, fx, cell, xn, S, _family_worst(ex, f, len(names)), _family_worst(eS, f, len(names)), f"grid N=20 path={path}")
    s.close()


# ---- 4. every plant kernel, from the inputs the device used ----------------------------------------------------------------------------------
def _nominal_solve(ba, s, B, seed=11):
    """one RTI step at nominal states, a few of them metres off: finite inputs, some at their bounds"""
    from bench import synthetic_inputs
    x0, circ = synthetic_inputs(B, seed=seed)
    x0[:max(B // 8, 1), :3] += np.array([8.0, -8.0, 5.0])
    s.set_x0(x0); s.set_yref(circ[:s.N + 1]); s.solve(sync=True)
    return circ


TRIG_DOMAIN = 1e6    # rad: sincos_pio2's specified range (bluerov2_model.hpp; test 1 above)

# Families whose run-time steps may miss the plain bar for a reason that is conditioning, not the kernel: the cause, and beside every figure
# the first-order bound that explains its size (_rounding_bound, computed with the exact model at the step's own inputs).
WIDER = {
    "kinks": "attitudes as in `wide`: a pitch of 1.27 rad with a yaw of 387 rad -- tan(theta) carries the roundings of psi (half an ulp at "
             "387: 3e-14 rad, four per step) into phi over the substeps",
    "far_yaw": "the state is rounded at |psi| of 1e3 .. 1e5 rad (half an ulp: up to 7e-12 rad) at every stage sum, and the next substep's "
               "sines and cosines see that",
    "steep_pitch": "1 / cos(theta) and tan(theta) at |theta| of 1.3 .. 1.5 rad, and beyond where the step moves on towards pi / 2: a rounding of "
                   "theta is carried on a hundred- to a thousandfold",
    "parameters": "m + added mass down to 1 kg with the solver's input on it (up to +-50): accelerations of thousands of m/s^2 and a damping "
                  "rate beyond what one ERK4 step integrates stably, so a rounding of a velocity grows within the period",
}


def _rounding_bound(exact, x, u, p, w, rp, dt, substeps, ref):
    """First-order bound of what rounding the state does to x+, per entry and scaled like the errors.  An ERK4 step in double rounds the
    state where it sums the stages -- once in the oracle's form x + h/6 (k1 + 2 k2 + 2 k3 + k4), four times in the device's, which adds
    stage by stage -- each time by up to half an ulp, 2^-53 |x_c|, of component c.  Carried to the end of the period to first order by
    d x+ / d x of the exact model at the step's own inputs (60 digits, central differences) and summed over the 4 x substeps roundings:
        B_j = sum_c |S_jc| 4 substeps 2^-53 max(|x_c|, |x+_c|) / max(1, |x+_j|)."""
    _, S = exact.sens(x, u, p, dt, w, rp, substeps)
    delta = 4.0 * substeps * 2.0 ** -53 * np.maximum(np.abs(x), np.abs(ref))
    return (np.abs(S[:, :12]) @ delta) / np.maximum(1.0, np.abs(ref))


def _hold_steps(what, oracle, exact, fx, fam, x, u, p, w, rp, dt, substeps, x1, wider=None):
    """EVERY x1[i] against the exact step from (x[i], u[i], p[i]) under w[i], rp[i]: scaled error <= FACTOR x max(the oracle's own worst
    error on the family's steps of this call, FLOOR).  A step of a family in WIDER that misses this has the first-order bound of
    _rounding_bound, entry by entry, added to it; no other family has, and no step is left out (wider: the families and causes of a test
    that has its own).  Two kinds of step have no bar, are counted in the record, and occur only in a loop that has already diverged by
    tens of orders of magnitude: one on which the ORACLE's step is not finite -- a double overflowed on the way, the oracle's error at
    those inputs is unbounded --, and one whose attitude angles (or rates times the period) leave |a| <= 1e6 rad, the range sincos_pio2
    is specified and tested for (beyond 2^31 quadrants its quadrant, beyond 1e15 rad its size is undefined, where libm's is not)."""
    wider = WIDER if wider is None else wider
    names = fx["names"]
    n = len(x)
    dev, orc, refs, lost = np.zeros((n, 12)), np.zeros((n, 12)), np.zeros((n, 12)), np.zeros(n, dtype=bool)
    for i in range(n):
        wi = None if w is None else w[i]
        ri = None if rp is None else rp[i]
        with np.errstate(all="ignore"):
            ref = refs[i] = exact.erk4(x[i], u[i], p[i], dt, wi, ri, substeps)
            fin = np.isfinite(ref)
            o = rk4_under_wrench(oracle, x[i], u[i], p[i], np.zeros(6) if wi is None else wi, dt, substeps, ri)
            dev[i] = np.where(fin, scaled_err(x1[i], np.where(fin, ref, 0.0)), np.where(np.isfinite(x1[i]), np.inf, 0.0))
            orc[i] = np.where(fin, scaled_err(o, np.where(fin, ref, 0.0)), 0.0)
            lost[i] = not np.all(np.isfinite(o))
            ang = max(np.abs(x[i][3:6]).max(), np.abs(ref[3:6]).max(), dt * np.abs(x[i][9:12]).max(), dt * np.abs(ref[9:12]).max())
            lost[i] = lost[i] or not ang <= TRIG_DOMAIN
    orc[lost] = 0.0
    dev[lost] = 0.0
    worst_orc = _family_worst(orc.max(axis=1), fam, len(names))
    parts, bad = [], []
    for fi in np.unique(fam):
        m = np.nonzero(fam == fi)[0]
        bar = FACTOR * max(float(worst_orc[fi]), FLOOR)
        worst = float(dev[m].max())
        text = f"{names[fi]} {worst:.2e} (oracle {float(worst_orc[fi]):.2e}, ratio {worst / (bar / FACTOR):.2f}"
        over = [i for i in m if not np.all(dev[i] <= bar)]
        if over and names[fi] in wider:
            used = 0.0
            for i in over:
                wi = None if w is None else w[i]
                ri = None if rp is None else rp[i]
                with np.errstate(all="ignore"):
                    B = _rounding_bound(exact, x[i], u[i], p[i], wi, ri, dt, substeps, refs[i])
                    ok = dev[i] <= bar + np.where(np.isfinite(B), B, np.inf)
                    used = max(used, float(np.max(np.where(dev[i] > bar, (dev[i] - bar) / B, 0.0))))
                if not np.all(ok):
                    bad.append((names[fi], int(i), float(dev[i].max()), bar, float(np.nanmax(B))))
            text += f"; {len(over)} of {len(m)} steps over the plain bar, at most {used:.3f} of their first-order rounding bound"
        elif over:
            bad.append((names[fi], [int(i) for i in over], worst, bar))
        parts.append(text + ")")
    _note(f"4 {what} ({n} steps{f', {int(lost.sum())} beyond double or the trig domain' if lost.any() else ''})", "; ".join(parts))
    assert not bad, (what, bad)


def _wrench_draw(fx, idx, rng):
    """the fixture's wrench where the case has one, else a draw of the same size: forces to 300, torques to 50"""
    ww = fx["ww"][idx].copy()
    none = ~ww.any(axis=1)
    ww[none] = np.concatenate([rng.uniform(-300, 300, (int(none.sum()), 3)), rng.uniform(-50, 50, (int(none.sum()), 3))], axis=1)
    return ww


@pytest.mark.parametrize("dist6", [False, True])
@pytest.mark.parametrize("mode", ["off", "constant", "table"])
def test_plant_step_from_fixture_states(ba, oracle, exact, fx, mode, dist6):
    """plant_kernel (no wrench) and plant_wrench_kernel (a constant wrench, a table with per-instance gains), substeps 1 and 4"""
    B, N = 64, 20
    rng = np.random.default_rng(5)
    idx = np.linspace(0, len(fx["h"]) - 1, B).astype(int)
    fam = fx["family"][idx]
    assert len(np.unique(fam)) == len(fx["names"])
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
    s.set_params(ba.P_NOMINAL)
    if dist6:
        s.enable_dist6()
    _nominal_solve(ba, s, B)
    u = s.results()["u0"].copy()
    assert np.all(np.isfinite(u)) and (np.abs(u) == 50.0).any() and (np.abs(u) < 50.0).any()
    x, p = fx["x"][idx], fx["p"][idx]
    s.set_plant_params(p)
    rp = None
    if dist6:
        rp = np.where(fx["rp"][idx].any(axis=1)[:, None], fx["rp"][idx], rng.uniform(-5, 5, (B, 2)))
        s.set_plant_rp_disturbance(rp)
    w = None
    if mode == "constant":
        s.set_plant_wrench(constant=_wrench_draw(fx, idx, rng))
    elif mode == "table":
        tab = np.concatenate([rng.uniform(-60, 60, (6, 3)), rng.uniform(-10, 10, (6, 3))], axis=1)
        gain = rng.uniform(-5, 5, B)
        s.set_plant_wrench(table=tab, gain=gain)
    for substeps in (1, 4):
        if mode != "off":
            s.plant_wrench_seek(3)
            w = s.plant_wrench(3)           # what the device's generator hands the plant at this tick
            assert w.shape == (B, 6) and np.abs(w).max() > 50.0 and np.abs(w).max(axis=1).min() > 0.0
        s.set_x0(x)
        s.plant_step(0.05, substeps)
        x1 = s.get_x0()
        kernel = "plant_kernel" if mode == "off" else f"plant_wrench_kernel {mode}"
        _hold_steps(f"{kernel}{' dist6' if dist6 else ''} substeps={substeps}", oracle, exact, fx, fam, x, u, p, w, rp, 0.05, substeps, x1)
    s.close()


@pytest.mark.parametrize("dist6", [False, True])
@pytest.mark.parametrize("substeps", [1, 2])
def test_plant_step_inside_the_one_launch_closed_loop(ba, oracle, exact, fx, substeps, dist6):
    """plant_step_wave: three ticks of brov_closed_loop in its one-launch form (fused kernel, trajectory table, no wrench) from fixture
    states; every logged x[k + 1] against the exact step from the logged x[k], u[k].  The controller, metres and
    radians away from its reference, saturates: most inputs sit at +-50 for all three ticks, whatever the family, and drive the speeds to
    tens of m/s, where the quadratic damping's rate times the step reaches ERK4's stability limit (2 x 18 x 20 / 13 x 0.05 = 2.8) and the
    state grows tick by tick.  So here every family may add the first-order rounding bound, for that one cause."""
    B, N, ticks = 48, 20, 3
    rng = np.random.default_rng(6)
    names = fx["names"]
    usable = np.nonzero(fx["family"] != names.index("world_wrench"))[0]
    idx = usable[np.linspace(0, len(usable) - 1, B).astype(int)]
    fam = fx["family"][idx]
    from bench import circle_trajectory
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05, kernel_path=ba.PATH_FUSED))
    s.set_params(ba.P_NOMINAL)
    rp = None
    if dist6:
        s.enable_dist6()
        rp = np.where(fx["rp"][idx].any(axis=1)[:, None], fx["rp"][idx], rng.uniform(-5, 5, (B, 2)))
        s.set_plant_rp_disturbance(rp)
    x, p = fx["x"][idx], fx["p"][idx]
    s.set_x0(x); s.set_plant_params(p); s.set_trajectory(circle_trajectory(256))
    ul, xl, sl = s.closed_loop(ticks, line0=0, ncols=16, dt=0.05, substeps=substeps)
    assert s.last_kernel_path() == ba.PATH_FUSED and np.array_equal(xl[0], x)
    assert (np.abs(ul) == 50.0).any()
    xs, us = xl[:-1].reshape(-1, 12), ul.reshape(-1, 4)
    _hold_steps(f"plant_step_wave{' dist6' if dist6 else ''} substeps={substeps}", oracle, exact, fx, np.tile(fam, ticks), xs, us, np.tile(p, (ticks, 1)), None,
                None if rp is None else np.tile(rp, (ticks, 1)), 0.05, substeps, xl[1:].reshape(-1, 12),
                wider={str(k): "inputs saturated at +-50 over three ticks: speeds of tens of m/s at ERK4's stability limit" for k in names})
    s.close()


@pytest.mark.parametrize("wrench", [False, True])
def test_fleet_plants_from_fixture_states(ba, oracle, exact, fx, wrench):
    """fleet_plant_kernel / fleet_plant_wrench_kernel: Fleet.step at 8 vehicles x 4 candidates, one vehicle per family, three rounds per substep count"""
    V, C, N = 8, 4, 20
    rng = np.random.default_rng(9)
    names, fam_all = fx["names"], fx["family"]
    s = ba.BatchSolver(V * C, ba.SolverOptions(N, 0.05))
    s.set_params(ba.P_NOMINAL)
    s.set_candidate_params("circle", np.tile(2.0 + 0.5 * np.arange(C) / C, V), np.full(V * C, 0.5), np.zeros(V * C))
    f = ba.Fleet(s, C)
    xv = np.zeros((V, 12)); xv[:, 0] = -2.2; xv[:, 2] = -20.0; xv[:, 5] = -0.5 * np.pi
    xv[:2, :3] += np.array([8.0, -8.0, 5.0])
    f.set_state(xv)
    s.set_yref_candidates_tick(0.0, 0.05); s.solve(sync=True)
    for substeps in (1, 4):
        X, U, P, W, X1, F = [], [], [], [], [], []
        for rnd in range(3):
            idx = np.array([np.nonzero((fam_all == fi) & (fx["h"] >= 0.05))[0][rnd] for fi in range(len(names))])
            x, p = fx["x"][idx], fx["p"][idx]
            f.set_plant_params(p)
            w = np.zeros((V, 6))
            if wrench:
                w = _wrench_draw(fx, idx, rng)
                f.set_wrench(constant=w)
            f.set_state(x)
            f.step(None, 0.05, substeps)
            u, _, _ = f.last()
            assert np.all(np.isfinite(u))
            X.append(x); U.append(u); P.append(p); W.append(w); X1.append(f.state()); F.append(fam_all[idx])
        _hold_steps(f"fleet_plant{'_wrench' if wrench else ''}_kernel substeps={substeps}", oracle, exact, fx, np.concatenate(F), np.concatenate(X),
                    np.concatenate(U), np.concatenate(P), np.concatenate(W) if wrench else None, None, 0.05, substeps, np.concatenate(X1))
    f.close(); s.close()
