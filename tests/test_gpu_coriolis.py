"""GPU tests of the plant's Coriolis stage (brov_coriolis_*, coriolis_eval_kernel, plant_coriolis_kernel) against
tests/coriolis_restatement.py, the oracle's model, and the call sequences the loops replace."""
import ctypes as C

import numpy as np
import pytest

from oracle import trajectory_oracle as T
import coriolis_restatement as CO
import current_restatement as CR
from current_restatement import CurrentRestatement
from thruster_restatement import ThrusterRestatement
from wrench_restatement import WrenchRestatement

pytestmark = pytest.mark.gpu
PERIODIC = dict(seed=0xC0FFEE123456789, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)
KA, MA = 0.3, 1.2481          # a roll added inertia that is not the reference's zero: the bx q product is exercised


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


def _loop_solver(ba, B, N, x0, traj, pp):
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(pp); s.set_trajectory(traj)
    return s


def _ekf(ba, B):
    """the device observer for the device plant, as tests/test_gpu_plant_wrench.py::_ekf_pair configures it"""
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
    return ba.BatchEkf(B, par)


def _set(s, terms, ka=KA, ma=MA):
    s.set_coriolis(rigid=bool(terms & 1), added=bool(terms & 2), ka=ka, ma=ma)
    assert s.coriolis_terms() == terms


def _same_bits(got, want):
    """equal as numbers where they are numbers, NaN where the other is NaN, and the zeros carry the same sign"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan]) and np.array_equal(np.signbit(got[~nan]), np.signbit(want[~nan]))


# ---- 1. the force, bit for bit ------------------------------------------------------------------------------------------------------------------
def test_the_force_matches_the_restatement_bit_for_bit(ba):
    B = 130                                                          # one full block plus two lanes
    rng = np.random.default_rng(3)
    s = ba.BatchSolver(B, ba.SolverOptions(10))
    p = np.tile(ba.P_NOMINAL, (B, 1)); p[:, 4:7] = rng.uniform(0.0, 8.0, (B, 3)); p[3, 5] = 0.0
    s.set_params(ba.P_NOMINAL); s.set_plant_params(p)
    x = rng.normal(size=(B, 12)) * 0.5
    x[:, 3:5] = rng.uniform(-0.5, 0.5, (B, 2)); x[:, 5] = rng.uniform(-7.0, 7.0, B)
    x[1, 6:12] = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0]                   # signed zeros: every product is a zero with a sign
    x[2, 9:11] = -0.0; x[4, 3:6] = 0.0; x[6, 6:9] = 0.0
    x[11, 6:12] = [0.0, -0.0, 0.0, 0.0, 0.0, 1.0]                    # (r v) - (q w) = (-0) - (+0): a negative zero on row X
    x[5, :] = np.nan; x[7, 7] = np.nan; x[8, 4] = np.nan             # a NaN row, a NaN velocity, a NaN attitude (felt through vc alone)
    vc = rng.uniform(-0.5, 0.5, (B, 3)); vc[9] = 0.0; vc[10, 2] = -0.0
    assert s.coriolis_terms() == 0 and not s.coriolis_eval(np.nan_to_num(x)).any()          # off: zeros
    seen = []
    for terms in (1, 2, 3):
        _set(s, terms)
        for water in (None, vc):
            got, want = s.coriolis_eval(x, water), CO.force_at(terms, x, p, water, KA, MA)
            assert _same_bits(got, want), (terms, water is not None, np.nonzero(~np.isclose(got, want, rtol=0, atol=0, equal_nan=True)))
            seen.append(got)
    assert np.isnan(seen[0][5, :3]).all() and seen[0][5, 3] == 0.0 and np.isnan(seen[5][5]).all()               # the NaN row; rigid has no yaw row
    assert not np.isnan(seen[0][8]).any() and np.isnan(seen[3][8, :3]).all()                                     # rigid ignores the attitude
    assert not np.array_equal(seen[2][0], seen[3][0]) and _same_bits(seen[0], seen[1])                          # the added group sees the water
    assert not seen[4][1].any() and seen[0][11, 0] == 0.0 and np.signbit(seen[0][11, 0])
    # one current for all, and the reference's coefficients as defaults
    s.set_coriolis(rigid=True, added=True)
    assert _same_bits(s.coriolis_eval(x, [0.1, -0.2, 0.05]), CO.force_at(3, x, p, np.tile([0.1, -0.2, 0.05], (B, 1)), 0.0, 1.2481))
    # evaluation moves nothing
    assert s.plant_wrench_tick() == 0 and not s.coriolis_last().any()
    with pytest.raises(RuntimeError, match="brov_coriolis_last_seconds: no plant step"):
        s.coriolis_last_seconds()
    s.coriolis_off()
    assert s.coriolis_terms() == 0 and not s.coriolis_eval(np.nan_to_num(x), vc).any()
    s.close()


# ---- 2. the plant step against the restated RK4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", [1, 3])
@pytest.mark.parametrize("substeps", [1, 4])
def test_plant_step_under_the_stage_matches_the_restated_rk4(ba, oracle, substeps, terms):
    """x0 and the bound of tests/test_gpu_current.py::test_plant_step_under_a_current_matches_the_restated_rk4 (1e-12 absolute against the
    same kind of restated RK4; measured there 3.6e-15 ... 1.8e-14), for the eight combinations of thruster stage, world wrench and current.
    Measured here: 3.6e-15 ... 1.4e-14."""
    N, B, tick = 20, 96, 13
    rng = np.random.default_rng(5)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * 0.1
    x0[:, 3:5] += rng.uniform(-0.4, 0.4, (B, 2))          # roll and pitch of a few tenths of a radian: the projection matters
    p = np.tile(ba.P_NOMINAL, (B, 1)); p[:, :4] = rng.uniform(-100, 100, (B, 4)); p[:, 4:7] += rng.uniform(0.0, 2.0, (B, 3))
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(p); s.set_yref(traj[:N + 1])
    s.solve()
    u0, t = s.results()["u0"], s.thrusts()
    vc = rng.uniform(-0.5, 0.5, (B, 3))
    lim = float(np.median(np.abs(t)))                     # about half of the commands clip
    gain = rng.uniform(0, 1, (B, 6))
    onset = np.where(np.arange(B) % 2 == 0, 5, 100)
    wr = WrenchRestatement(B).periodic(**PERIODIC)
    _set(s, terms)
    worst = 0.0
    for th in (False, True):
        for wrench in (False, True):
            for current in (False, True):
                name = f"terms {terms}, thrusters {th}, wrench {wrench}, current {current}, substeps {substeps}"
                s.set_plant_wrench(periodic=PERIODIC) if wrench else s.plant_wrench_off()
                s.set_current(constant=vc) if current else s.current_off()
                g = a = None
                if th:
                    s.set_thrusters(lo=-lim, hi=lim, gain=gain, onset=onset)
                    rt = ThrusterRestatement(B, None, -lim, lim, gain, None, onset)
                    a, g = rt.step(tick, t)
                else:
                    s.thrusters_off()
                s.set_x0(x0); s.plant_wrench_seek(tick)
                s.plant_step(0.05, substeps)
                x1 = s.get_x0()
                assert s.plant_wrench_tick() == tick + 1, name
                w = wr.wrench(tick) if wrench else None
                water = vc if current else None
                err = np.abs(x1 - CO.plant_step(oracle, x0, u0, p, w, water, terms, 0.05, substeps, KA, MA, g=g)).max()
                print(f"{name}: |x_gpu - x_restated|_inf = {err:.2e}")
                worst = max(worst, err)
                assert err < 1e-12, (name, err)
                # ... and the stage is felt: the same step without it lands elsewhere
                without = CR.plant_step(oracle, x0, u0, p, w, np.zeros((B, 3)) if water is None else water, 0.05, substeps, g=g)
                assert np.abs(x1 - without).max() > 1e-6, name
                # the force at the start state, as the evaluation gives it
                assert _same_bits(s.coriolis_last(), CO.force_at(terms, x0, p, water, KA, MA)), name
                if current:
                    assert np.array_equal(s.current_last(), vc), name
                if th:
                    st = s.thruster_stats()
                    assert np.array_equal(s.thruster_last(), a) and st["steps"] == 1, name
                    assert np.array_equal(st["clip_ticks"], rt.clip_ticks) and np.array_equal(st["lost_sq"], rt.lost_sq), name
    print(f"terms {terms}, substeps {substeps}: worst |x_gpu - x_restated|_inf over the eight combinations = {worst:.2e}")
    assert 0.0 < s.coriolis_last_seconds() < 1.0
    s.close()


# ---- 3. off is the parent path --------------------------------------------------------------------------------------------------------------
def test_off_is_the_parent_path(ba):
    N, B, ticks = 20, 48, 8
    rng = np.random.default_rng(8)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = rng.uniform(-100, 100, (B, 4))
    parent = _loop_solver(ba, B, N, x0, traj, pp)          # never touches the stage's API
    off = _loop_solver(ba, B, N, x0, traj, pp)
    _set(off, 3); off.coriolis_off()
    on = _loop_solver(ba, B, N, x0, traj, pp)
    _set(on, 1)
    assert parent.coriolis_terms() == off.coriolis_terms() == 0 and on.coriolis_terms() == 1
    for s in (parent, off, on):
        s.set_yref(traj[:N + 1]); s.solve(); s.plant_step(0.05, 2)
    assert parent.get_x0().tobytes() == off.get_x0().tobytes() and not np.array_equal(parent.get_x0(), on.get_x0())
    assert not off.coriolis_last().any()
    for s in (parent, off, on):
        s.set_x0(x0); s.init_iterate_default()
    lp, lo, ln = parent.closed_loop(ticks, line0=3), off.closed_loop(ticks, line0=3), on.closed_loop(ticks, line0=3)
    assert parent.last_kernel_path() == off.last_kernel_path() == ba.PATH_FUSED
    for a, b in zip(lp, lo):
        assert a.tobytes() == b.tobytes()
    assert parent.get_x0().tobytes() == off.get_x0().tobytes() and np.array_equal(parent.results(), off.results())
    assert not np.array_equal(lp[1], ln[1]) and np.all(ln[2] == 0)
    assert parent.plant_wrench_tick() == off.plant_wrench_tick() == on.plant_wrench_tick() == ticks + 1
    with pytest.raises(RuntimeError, match="brov_coriolis_last_seconds: no plant step"):
        off.coriolis_last_seconds()
    for s in (parent, off, on):
        s.close()


def test_the_other_stages_bookkeeping_does_not_depend_on_the_kernel_that_keeps_it(ba):
    """the same solve, the same thruster stage, wrench and current: three plant steps by plant_current_kernel, three by plant_coriolis_kernel"""
    N, B = 20, 96
    rng = np.random.default_rng(14)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0 += rng.normal(size=(B, 12)) * 0.1
    gain, bias = rng.uniform(0, 1, (B, 6)), rng.uniform(-5, 5, (B, 6))
    tab = rng.uniform(-0.5, 0.5, (5, 3))
    out = []
    for stage in (False, True):
        s = ba.BatchSolver(B, ba.SolverOptions(N))
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_yref(traj[:N + 1])
        s.solve()
        lim = float(np.median(np.abs(s.thrusts())))
        s.set_thrusters(lo=-lim, hi=lim, gain=gain, bias=bias, onset=np.arange(B) % 3)
        s.set_plant_wrench(periodic=PERIODIC)
        s.set_current(table=tab, gain=np.linspace(0.5, 1.5, B))
        if stage:
            _set(s, 3)
        for _ in range(3):
            s.plant_step(0.05, 1)
        out.append((s.thruster_stats(), s.thruster_last(), s.get_x0(), s.thruster_last_seconds(), s.current_last(), s.current_last_seconds()))
        s.close()
    (sa, la, xa, ta, ca, tca), (sb, lb, xb, tb, cb, tcb) = out
    assert sa["steps"] == sb["steps"] == 3 and sa["clip_ticks"].sum() > 0 and sa["lost_sq"].min() > 0.0
    assert np.array_equal(sa["clip_ticks"], sb["clip_ticks"]) and np.array_equal(sa["lost_sq"], sb["lost_sq"]) and np.array_equal(la, lb)
    assert np.array_equal(ca, cb) and np.array_equal(ca, tab[2][None, :] * np.linspace(0.5, 1.5, B)[:, None])
    assert np.abs(xa - xb).max() > 1e-6 and all(0.0 < t < 1.0 for t in (ta, tb, tca, tcb))


# ---- 4. the Gauss-Markov current under the stage ----------------------------------------------------------------------------------------------
def test_gauss_markov_state_is_byte_identical_after_64_plant_steps_under_the_stage(ba):
    N, B = 20, 96
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_yref(traj[:N + 1])
    s.solve()
    _set(s, 3)
    mean = CR.gm_case_mean(B)
    s.set_current(gauss_markov=dict(mean=mean, **CR.GM_CASE))
    r = CurrentRestatement(B).gauss_markov(mean=mean, **CR.GM_CASE)
    s.plant_wrench_seek(CR.GM_TICK0)
    jump = np.random.default_rng(6).uniform(-0.6, 0.6, (B, 3))       # beyond the bounds too: the next advance clamps it
    for k in range(CR.GM_TICK0, CR.GM_TICK0 + CR.GM_STEPS):
        if k == CR.GM_TICK0 + 30:
            s.set_current_state(jump); r.set_state(jump)
        s.plant_step(0.05, 1)
        want = r.step(k)
        if k % 8 == 0 or k == CR.GM_TICK0 + 30:
            assert np.array_equal(s.current_last(), want), k
            assert s.current_state().tobytes() == r.state(k + 1).tobytes(), k
    assert s.current_state().tobytes() == r.state(0).tobytes()
    assert s.plant_wrench_tick() == CR.GM_TICK0 + CR.GM_STEPS and np.isfinite(s.get_x0()).all()
    assert (r.clamped_lo.sum(0) >= 1).all() and (r.clamped_hi.sum(0) >= 1).all()
    assert 0.0 < s.coriolis_last_seconds() < 1.0 and 0.0 < s.current_last_seconds() < 1.0 and np.abs(s.coriolis_last()).max() > 0.0
    s.close()


# ---- 5. the loops equal their call sequences, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "dob", "delayed"])
def test_loops_under_the_stage_equal_their_call_sequences(ba, kind):
    """plain: both groups, behind a faulty thruster stage in a Gauss-Markov current; dob: the rigid group under the periodic wrench, the
    observer closing the loop; delayed: both groups behind the delay stage (2 steps) and the rotor stage"""
    N, B, ticks, line0, tick0 = 20, 24, 12, 1, 40
    rng = np.random.default_rng(12)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :6] += rng.normal(size=(B, 6)) * 0.03
    pp = np.tile(ba.P_NOMINAL, (B, 1))
    mean = CR.gm_case_mean(B)

    def solver():
        s = _loop_solver(ba, B, N, x0, traj, pp)
        if kind == "plain":
            gain = np.ones((B, 6)); gain[::2, 0] = 0.0
            s.set_thrusters(lo=-100.0, hi=100.0, gain=gain, onset=tick0 + 4)
            s.set_current(gauss_markov=dict(mean=mean, **CR.GM_CASE))
        elif kind == "dob":
            s.set_plant_wrench(periodic=PERIODIC)
        else:
            s.set_delay(2); s.set_rotors(tau=0.1)
        _set(s, 1 if kind == "dob" else 3)
        s.plant_wrench_seek(tick0)
        return s, (_ekf(ba, B) if kind == "dob" else None)

    def loop(s, e):
        if kind != "dob":
            ul, xl, sl, wl = s.closed_loop(ticks, line0=line0, log_wrench=True)
            return dict(u=ul, x=xl, status=sl, wrench=wl)
        return s.closed_loop_dob(e, ticks=ticks, line0=line0)

    def end(s, e):
        return (s.get_x0(), s.coriolis_last(), s.get_params(), s.current_state(), e.state() if e else (), s.plant_wrench_tick())

    # the loop in one call
    s, e = solver()
    la = loop(s, e)
    end_a = end(s, e)
    # ... and as its public call sequence
    q, eq = solver()
    lb = dict(u=[], x=[q.get_x0()], status=[], wrench=[], est=[])
    for k in range(ticks):
        q.set_yref_from_trajectory(line0 + k, 16); q.solve()
        lb["wrench"].append(q.plant_wrench(q.plant_wrench_tick()))
        xk = q.get_x0()
        q.plant_step(0.05, 1)
        if kind == "dob":                                            # still water, no delay: the force at the state the step started from
            assert _same_bits(q.coriolis_last(), CO.force_at(1, xk, pp, None, KA, MA)), k
            eq.update_from_solver(q); eq.apply_to_solver(q)
            lb["est"].append(eq.state()[0][:, 12:].copy())
        res = q.results()
        lb["u"].append(res["u0"].copy()); lb["status"].append(res["status"].copy()); lb["x"].append(q.get_x0())
    lb = {k: np.array(v) for k, v in lb.items() if len(v)}
    end_b = end(q, eq)
    assert set(la) >= set(lb)
    for key in lb:
        assert la[key].tobytes() == lb[key].tobytes(), key
    for a, b in zip(end_a[:4], end_b[:4]):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(end_a[4], end_b[4]):
        assert np.array_equal(a, b)
    assert end_a[5] == end_b[5] == tick0 + ticks and np.all(la["status"] == 0)
    assert np.abs(la["x"][1:] - la["x"][:-1]).max() > 1e-3 and np.abs(end_a[1]).max() > 0.0
    if kind == "plain":
        assert s.thruster_stats()["steps"] == ticks and np.array_equal(s.thruster_stats()["lost_sq"], q.thruster_stats()["lost_sq"])
    # the scored loop: the tracker's records do not depend on how the run is cut, and its plant is the logged loop's
    recs = []
    for chunk in (5, 0):
        s.set_x0(x0); s.init_iterate_default(); s.set_params(ba.P_NOMINAL); s.set_plant_params(pp)
        s.plant_wrench_seek(tick0)
        if kind == "plain":
            s.set_current_state(mean)
        if kind == "delayed":
            s.set_delay(2); s.set_rotors(tau=0.1)                    # the queue and the rotor state start afresh
        e2 = _ekf(ba, B) if kind == "dob" else None
        t = ba.BatchTrack(B)
        s.closed_loop_track(t, ticks, line0=line0, ekf=e2, chunk=chunk)
        recs.append((t.stats().tobytes(), s.get_x0(), s.coriolis_last()))
        t.close()
        if e2 is not None:
            e2.close()
    assert recs[0][0] == recs[1][0] and np.array_equal(recs[0][1], recs[1][1]) and np.array_equal(recs[0][2], recs[1][2])
    if kind != "dob":
        assert np.array_equal(recs[0][1], end_a[0]) and np.array_equal(recs[0][2], end_a[1])
    for o in (s, q, e, eq):
        if o is not None:
            o.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_change_nothing_and_the_fleet_refuses_the_stage(ba):
    B, N = 4, 10
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
    s.set_params(ba.P_NOMINAL)
    L, h = s._L, s._h
    terms, ka, ma = C.c_int(-1), C.c_double(-1.0), C.c_double(-1.0)
    assert L.brov_coriolis_get(h, C.byref(terms), C.byref(ka), C.byref(ma)) == 0 and (terms.value, ka.value, ma.value) == (0, 0.0, 1.2481)
    _set(s, 2, 0.25, 0.75)
    s.plant_wrench_seek(5)

    def unchanged():
        assert L.brov_coriolis_get(h, C.byref(terms), C.byref(ka), C.byref(ma)) == 0
        return (terms.value, ka.value, ma.value) == (2, 0.25, 0.75) and s.coriolis_terms() == 2 and s.plant_wrench_tick() == 5

    assert unchanged()
    for args, text in (((0, 0.0, 1.0), "brov_coriolis_set: terms must be"), ((4, 0.0, 1.0), "brov_coriolis_set: terms must be"),
                       ((-1, 0.0, 1.0), "brov_coriolis_set: terms must be"), ((1, np.nan, 1.0), "brov_coriolis_set: ka and ma must be finite"),
                       ((1, -0.1, 1.0), "brov_coriolis_set: ka and ma"), ((1, np.inf, 1.0), "brov_coriolis_set: ka and ma"),
                       ((3, 0.0, np.nan), "brov_coriolis_set: ka and ma"), ((3, 0.0, -1.0), "brov_coriolis_set: ka and ma"),
                       ((3, 0.0, -np.inf), "brov_coriolis_set: ka and ma")):
        assert L.brov_coriolis_set(h, args[0], args[1], args[2]) == -1, args
        assert L.brov_last_error().decode().startswith(text), (args, L.brov_last_error())
        assert unchanged(), args
    with pytest.raises(RuntimeError, match="brov_coriolis_set: terms must be"):
        s.set_coriolis(rigid=False, added=False)
    assert unchanged()
    dp = C.POINTER(C.c_double)
    ok = np.zeros((B, 12)).ctypes.data_as(dp)
    raw = [("brov_coriolis_eval_host", (h, None, None, ok)), ("brov_coriolis_eval_host", (h, ok, None, None)), ("brov_coriolis_last_host", (h, None)),
           ("brov_coriolis_last_seconds", (h, None)), ("brov_coriolis_get", (h, None, C.byref(ka), C.byref(ma))),
           ("brov_coriolis_get", (h, C.byref(terms), None, C.byref(ma))), ("brov_coriolis_get", (h, C.byref(terms), C.byref(ka), None))]
    for name, args in raw:
        assert getattr(L, name)(*args) == -1, name
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())
        assert unchanged(), name
    with pytest.raises(ValueError):
        s.coriolis_eval(np.zeros((B, 11)))
    # the fleet has its own plant kernel, which does not know the stage
    x0 = np.zeros((B, 12)); x0[:, 2] = -20.0
    s.plant_wrench_seek(0)
    s.set_x0(x0); s.set_candidate_params("circle", np.full(B, 2.0), np.full(B, 0.5), np.zeros(B))
    f = ba.Fleet(s, 2)
    for name, call in (("brov_fleet_step", lambda: f.step()), ("brov_closed_loop_fleet", lambda: f.closed_loop(2, dt_ref=0.05, dt_node=0.05)),
                       ("brov_closed_loop_fleet_dob", lambda: f.closed_loop_dob(None, 2, dt_ref=0.05, dt_node=0.05))):
        with pytest.raises(RuntimeError, match=name + r": the Coriolis stage of the solver's plant is on \(brov_coriolis_set\)"):
            call()
    assert np.array_equal(s.get_x0(), x0) and s.plant_wrench_tick() == 0
    s.coriolis_off()
    u, x, st, win = f.closed_loop(2, dt_ref=0.05, dt_node=0.05)
    assert np.isfinite(x).all()
    f.close(); s.close()


# ---- 7. the point of it -------------------------------------------------------------------------------------------------------------------------
def test_the_phantom_disturbance_goes_with_the_rigid_body_terms_on_the_device(ba, oracle):
    """The scenario of tests/test_coriolis_cpu.py::test_the_phantom_disturbance_goes_with_the_rigid_body_terms on the device: B = 4, N = 20,
    80 ticks of brov_closed_loop_dob, no external disturbance; median |estimate| over the last 20 ticks.  The three assertions of the CPU
    test, and the device's medians within 1e-6 relative of the CPU loop's (X, Y and N, the three the assertions use)."""
    N, B, ticks = 20, 4, 80
    traj, x0 = CO.scenario_inputs(B)
    pp = np.tile(ba.P_NOMINAL, (B, 1))
    med, cpu = {}, {}
    for terms in (0, 1, 3):
        s = _loop_solver(ba, B, N, x0, traj, pp)
        if terms:
            s.set_coriolis(rigid=True, added=bool(terms & 2))        # the reference's coefficients: ka = 0, ma = 1.2481
        e = _ekf(ba, B)
        log = s.closed_loop_dob(e, ticks=ticks)
        assert np.all(log["status"] == 0) and np.isfinite(log["x"]).all()
        med[terms] = CO.phantom_medians(log["est"])
        c = CO.cpu_dob_loop(oracle, CO.ekf_for_the_device_plant(), terms, traj, x0, ba.P_NOMINAL, pp, N, ticks)
        cpu[terms] = CO.phantom_medians(c["est"])
        rel = np.abs(med[terms] - cpu[terms])[[0, 1, 5]] / cpu[terms][[0, 1, 5]]
        print(f"terms {terms}: median |estimate| X {med[terms][0]:.6f} N, Y {med[terms][1]:.6f} N, N {med[terms][5]:.6f} N m; "
              f"relative to the CPU loop's {rel[0]:.2e}, {rel[1]:.2e}, {rel[2]:.2e}; |dx| = {np.abs(log['x'] - c['x']).max():.2e}")
        s.close(); e.close()
    off, rigid, both = med[0], med[1], med[3]
    assert off[0] > 1.0 and off[1] > 1.0
    assert rigid[0] < 0.1 * off[0] and rigid[1] < 0.1 * off[1]
    assert both[5] > 10.0 * rigid[5]
    for terms in (0, 1, 3):
        assert (np.abs(med[terms] - cpu[terms])[[0, 1, 5]] <= 1e-6 * cpu[terms][[0, 1, 5]]).all(), (terms, med[terms], cpu[terms])
