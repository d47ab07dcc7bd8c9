"""GPU tests of the plant's ocean current (brov_current_*, current_eval_kernel, plant_current_kernel) against tests/current_restatement.py,
the oracle's model, and the call sequences the loops replace."""
import ctypes as C

import numpy as np
import pytest

from oracle import trajectory_oracle as T
import current_restatement as CR
from current_restatement import CurrentRestatement
from thruster_restatement import ThrusterRestatement
from wrench_restatement import WrenchRestatement

pytestmark = pytest.mark.gpu
PERIODIC = dict(seed=0xC0FFEE123456789, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)


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


def _gm(s, B):
    """the Gauss-Markov case of current_restatement.py on the device and restated"""
    mean = CR.gm_case_mean(B)
    s.set_current(gauss_markov=dict(mean=mean, **CR.GM_CASE))
    return CurrentRestatement(B).gauss_markov(mean=mean, **CR.GM_CASE)


# ---- 1. the generator, bit for bit ----------------------------------------------------------------------------------------------------------
def test_constant_and_table_match_the_restatement_bit_for_bit(ba):
    B = 130                                                          # one full block plus two lanes
    rng = np.random.default_rng(3)
    s = ba.BatchSolver(B, ba.SolverOptions(10))
    assert s.current_mode() == ba.CURRENT_OFF and not s.current(3).any() and not s.current_state().any()
    vc = rng.uniform(-0.5, 0.5, (B, 3)); vc[1, 1] = 0.0; vc[2, 2] = -0.0
    tab, gain = rng.uniform(-0.5, 0.5, (7, 3)), rng.uniform(-3, 3, B)
    for name, kw, r, mode in (("constant", dict(constant=vc), CurrentRestatement(B).constant(vc), ba.CURRENT_CONSTANT),
                              ("table", dict(table=tab), CurrentRestatement(B).table(tab), ba.CURRENT_TABLE),
                              ("table with gain", dict(table=tab, gain=gain), CurrentRestatement(B).table(tab, gain), ba.CURRENT_TABLE)):
        s.set_current(**kw)
        assert s.current_mode() == mode
        for tick in (0, 3, 6, 7, 100000):
            got, want = s.current(tick), r.current(tick)
            assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), (name, tick)
        assert np.array_equal(s.current_state(), r.current(0))       # what the next step, at tick 0, applies
    assert not np.array_equal(s.current(0), s.current(1)) and np.array_equal(s.current(6), s.current(9))
    # one current for all
    s.set_current(constant=[0.1, -0.2, 0.05])
    assert np.array_equal(s.current(4), np.tile([0.1, -0.2, 0.05], (B, 1)))
    # evaluation moves nothing
    assert s.plant_wrench_tick() == 0 and not s.current_last().any()
    s.current_off()
    assert s.current_mode() == ba.CURRENT_OFF and not s.current(3).any()
    s.close()


def test_gauss_markov_state_is_byte_identical_after_64_plant_steps(ba):
    N, B = 20, 96
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_yref(traj[:N + 1])
    s.solve()
    r = _gm(s, B)
    assert s.current_mode() == ba.CURRENT_GAUSS_MARKOV and np.array_equal(s.current_state(), r.mean)
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
    assert (r.clamped_lo.sum(0) >= 1).all() and (r.clamped_hi.sum(0) >= 1).all()     # (tests/test_current_cpu.py: a property of the inputs)
    # the seek moves the noise counter only: the state stays, and the same tick draws the same noise
    c = s.current_state()
    s.plant_wrench_seek(CR.GM_TICK0)
    assert np.array_equal(s.current_state(), c)
    r2 = CurrentRestatement(B).gauss_markov(mean=r.mean, **CR.GM_CASE); r2.set_state(c)
    s.plant_step(0.05, 1); r2.step(CR.GM_TICK0)
    assert s.current_state().tobytes() == r2.state(0).tobytes()
    assert 0.0 < s.current_last_seconds() < 1.0
    s.close()


# ---- 2. the plant step against the restated RK4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 4])
def test_plant_step_under_a_current_matches_the_restated_rk4(ba, oracle, substeps):
    """x0 as in tests/test_gpu_plant_wrench.py::test_plant_step_under_a_wrench_matches_the_restated_rk4, with that test's own bound, for the
    four combinations of thruster stage and world wrench"""
    N, B, tick = 20, 96, 13
    rng = np.random.default_rng(5)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * 0.1
    x0[:, 3:5] += rng.uniform(-0.4, 0.4, (B, 2))          # roll and pitch of a few tenths of a radian: the projection matters
    p = np.tile(ba.P_NOMINAL, (B, 1)); p[:, :4] = rng.uniform(-100, 100, (B, 4))
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(p); s.set_yref(traj[:N + 1])
    s.solve()
    u0, t = s.results()["u0"], s.thrusts()
    vc = rng.uniform(-0.5, 0.5, (B, 3))
    assert np.abs(vc).max() > 0.45
    lim = float(np.median(np.abs(t)))                     # about half of the commands clip
    gain = rng.uniform(0, 1, (B, 6))
    onset = np.where(np.arange(B) % 2 == 0, 5, 100)
    wr = WrenchRestatement(B).periodic(**PERIODIC)
    s.set_current(constant=vc)
    for th in (False, True):
        for wrench in (False, True):
            name = f"thrusters {th}, wrench {wrench}, substeps {substeps}"
            if wrench:
                s.set_plant_wrench(periodic=PERIODIC)
            else:
                s.plant_wrench_off()
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
            assert s.plant_wrench_tick() == tick + 1 and np.array_equal(s.current_last(), vc), name
            w = wr.wrench(tick) if wrench else None
            err = np.abs(x1 - CR.plant_step(oracle, x0, u0, p, w, vc, 0.05, substeps, g=g)).max()
            print(f"{name}: |x_gpu - x_restated|_inf = {err:.2e}")
            assert err < 1e-12, (name, err)
            # ... and the current is felt: the same step in still water lands elsewhere
            still = CR.plant_step(oracle, x0, u0, p, w, np.zeros((B, 3)), 0.05, substeps, g=g)
            assert np.abs(x1 - still).max() > 1e-6, name
            if th:
                st = s.thruster_stats()
                assert np.array_equal(s.thruster_last(), a) and st["steps"] == 1, name
                assert np.array_equal(st["clip_ticks"], rt.clip_ticks) and np.array_equal(st["lost_sq"], rt.lost_sq), name
    s.close()


# ---- 3. off is the parent path; a zero current agrees with it -------------------------------------------------------------------------------
def test_mode_off_is_the_parent_path_and_a_zero_current_agrees_with_it(ba):
    N, B, ticks = 20, 48, 8
    rng = np.random.default_rng(8)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = rng.uniform(-100, 100, (B, 4))
    parent = _loop_solver(ba, B, N, x0, traj, pp)          # never touches the current API
    off = _loop_solver(ba, B, N, x0, traj, pp)
    off.set_current(constant=rng.uniform(-0.5, 0.5, (B, 3))); _gm(off, B); off.current_off()
    zero = _loop_solver(ba, B, N, x0, traj, pp)
    zero.set_current(constant=np.zeros(3))
    assert parent.current_mode() == off.current_mode() == ba.CURRENT_OFF and zero.current_mode() == ba.CURRENT_CONSTANT
    for s in (parent, off, zero):
        s.set_yref(traj[:N + 1]); s.solve(); s.plant_step(0.05, 2)
    xp, xo, xz = parent.get_x0(), off.get_x0(), zero.get_x0()
    assert np.array_equal(xp, xo)
    print(f"zero current against the parent path, one step: |dx| = {np.abs(xz - xp).max():.2e}")
    assert np.abs(xz - xp).max() < 1e-12
    for s in (parent, off, zero):
        s.set_x0(x0); s.init_iterate_default()
    lp = parent.closed_loop(ticks, line0=3)
    lo = off.closed_loop(ticks, line0=3, log_wrench=True)
    lz = zero.closed_loop(ticks, line0=3, log_wrench=True)
    assert parent.last_kernel_path() == off.last_kernel_path() == ba.PATH_FUSED
    for a, b in zip(lp, lo[:3]):
        assert np.array_equal(a, b)
    assert not lo[3].any() and not lz[3].any()
    assert np.array_equal(parent.get_x0(), off.get_x0()) and np.array_equal(parent.results(), off.results())
    assert np.array_equal(lp[2], lz[2])
    print(f"zero current against the parent path, {ticks} ticks: |du| = {np.abs(lp[0] - lz[0]).max():.2e}, |dx| = {np.abs(lp[1] - lz[1]).max():.2e}")
    assert np.abs(lp[0] - lz[0]).max() < 1e-12 and np.abs(lp[1] - lz[1]).max() < 1e-12
    assert parent.plant_wrench_tick() == off.plant_wrench_tick() == zero.plant_wrench_tick() == ticks + 1
    with pytest.raises(RuntimeError, match="brov_current_last_seconds: no plant step"):
        off.current_last_seconds()
    for s in (parent, off, zero):
        s.close()


def test_thruster_statistics_do_not_depend_on_the_kernel_that_keeps_them(ba):
    """the same solve, the same thruster stage: one plant step by plant_thruster_kernel, one by plant_current_kernel"""
    N, B = 20, 96
    rng = np.random.default_rng(14)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0 += rng.normal(size=(B, 12)) * 0.1
    gain, bias = rng.uniform(0, 1, (B, 6)), rng.uniform(-5, 5, (B, 6))
    out = []
    for current in (False, True):
        s = ba.BatchSolver(B, ba.SolverOptions(N))
        s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_yref(traj[:N + 1])
        s.solve()
        lim = float(np.median(np.abs(s.thrusts())))
        s.set_thrusters(lo=-lim, hi=lim, gain=gain, bias=bias, onset=np.arange(B) % 3)
        s.set_plant_wrench(periodic=PERIODIC)
        if current:
            s.set_current(constant=rng.uniform(-0.5, 0.5, (B, 3)))
        for _ in range(3):
            s.plant_step(0.05, 1)
        out.append((s.thruster_stats(), s.thruster_last(), s.get_x0(), s.thruster_last_seconds()))
        s.close()
    (sa, la, xa, ta), (sb, lb, xb, tb) = out
    assert sa["steps"] == sb["steps"] == 3 and sa["clip_ticks"].sum() > 0 and sa["lost_sq"].min() > 0.0
    assert np.array_equal(sa["clip_ticks"], sb["clip_ticks"]) and np.array_equal(sa["lost_sq"], sb["lost_sq"]) and np.array_equal(la, lb)
    assert np.abs(xa - xb).max() > 1e-6 and 0.0 < ta < 1.0 and 0.0 < tb < 1.0


# ---- 4. the loops equal their call sequences, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "dob"])
def test_loops_under_a_current_equal_their_call_sequences(ba, kind):
    """Gauss-Markov current; plain: behind a faulty thruster stage; dob: under the periodic wrench, the observer closing the loop"""
    N, B, ticks, line0, tick0 = 20, 24, 12, 1, 40
    rng = np.random.default_rng(12)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :6] += rng.normal(size=(B, 6)) * 0.03
    pp = np.tile(ba.P_NOMINAL, (B, 1))

    def solver():
        s = _loop_solver(ba, B, N, x0, traj, pp)
        if kind == "plain":
            gain = np.ones((B, 6)); gain[::2, 0] = 0.0
            s.set_thrusters(lo=-100.0, hi=100.0, gain=gain, onset=tick0 + 4)
        else:
            s.set_plant_wrench(periodic=PERIODIC)
        r = _gm(s, B)
        s.plant_wrench_seek(tick0)
        return s, r, (_ekf(ba, B) if kind == "dob" else None)

    def loop(s, e):
        if kind == "plain":
            ul, xl, sl, wl = s.closed_loop(ticks, line0=line0, log_wrench=True)
            return dict(u=ul, x=xl, status=sl, wrench=wl)
        return s.closed_loop_dob(e, ticks=ticks, line0=line0)

    # the loop in one call
    s, r, e = solver()
    la = loop(s, e)
    end_a = (s.get_x0(), s.current_state(), s.current_last(), s.get_params(), e.state() if e else (), s.plant_wrench_tick())
    # ... and as its public call sequence, the current of every tick against the restatement
    q, rq, eq = solver()
    lb = dict(u=[], x=[q.get_x0()], status=[], wrench=[], est=[])
    for k in range(ticks):
        q.set_yref_from_trajectory(line0 + k, 16); q.solve()
        tick = q.plant_wrench_tick()
        lb["wrench"].append(q.plant_wrench(tick))
        q.plant_step(0.05, 1)
        assert np.array_equal(q.current_last(), rq.step(tick)), k
        if eq is not None:
            eq.update_from_solver(q); eq.apply_to_solver(q)
            lb["est"].append(eq.state()[0][:, 12:].copy())
        res = q.results()
        lb["u"].append(res["u0"].copy()); lb["status"].append(res["status"].copy()); lb["x"].append(q.get_x0())
    lb = {k: np.array(v) for k, v in lb.items() if len(v)}
    end_b = (q.get_x0(), q.current_state(), q.current_last(), q.get_params(), eq.state() if eq else (), q.plant_wrench_tick())
    assert set(la) >= set(lb)
    for key in lb:
        assert np.array_equal(la[key], lb[key]), key
    for a, b in zip(end_a[:4], end_b[:4]):
        assert np.array_equal(a, b)
    for a, b in zip(end_a[4], end_b[4]):
        assert np.array_equal(a, b)
    assert end_a[5] == end_b[5] == tick0 + ticks and np.all(la["status"] == 0)
    assert end_a[1].tobytes() == rq.state(0).tobytes()                 # the Gauss-Markov state behind the loop is the restatement's
    assert np.abs(la["x"][1:] - la["x"][:-1]).max() > 1e-3
    if kind == "plain":
        assert not la["wrench"].any() and s.thruster_stats()["steps"] == ticks
        assert np.array_equal(s.thruster_stats()["lost_sq"], q.thruster_stats()["lost_sq"])
    else:
        assert np.abs(la["wrench"]).max() > 1.0
    # the scored loop: the tracker's records and the Gauss-Markov state do not depend on how the run is cut
    recs = []
    for chunk in (5, 0):
        s.set_x0(x0); s.init_iterate_default(); s.set_params(ba.P_NOMINAL); s.set_plant_params(pp)
        s.plant_wrench_seek(tick0); s.set_current_state(r.mean)
        e2 = _ekf(ba, B) if kind == "dob" else None
        t = ba.BatchTrack(B)
        s.closed_loop_track(t, ticks, line0=line0, ekf=e2, chunk=chunk)
        recs.append((t.stats().tobytes(), s.get_x0(), s.current_state()))
        t.close()
        if e2 is not None:
            e2.close()
    assert recs[0][0] == recs[1][0] and np.array_equal(recs[0][1], recs[1][1]) and np.array_equal(recs[0][2], recs[1][2])
    assert np.array_equal(recs[0][2], end_a[1])                        # the state's path does not depend on the plant's: the logged loop's
    if kind == "plain":
        assert np.array_equal(recs[0][1], end_a[0])
    for o in (s, q, e, eq):
        if o is not None:
            o.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_change_nothing_and_the_fleet_refuses_a_current(ba):
    B, N = 4, 10
    rng = np.random.default_rng(2)
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
    s.set_params(ba.P_NOMINAL)
    with pytest.raises(RuntimeError, match="brov_current_set_state_host: only the Gauss-Markov"):
        s.set_current_state(np.zeros(3))
    mean = rng.uniform(-0.2, 0.2, (B, 3))
    gm = dict(seed=5, mean=mean, mu=0.5, amp=0.02, lo=-0.3, hi=0.3, step=0.05)
    s.set_current(gauss_markov=gm)
    c0 = rng.uniform(-0.2, 0.2, (B, 3))
    s.set_current_state(c0); s.plant_wrench_seek(5)

    def unchanged():
        return s.current_mode() == ba.CURRENT_GAUSS_MARKOV and np.array_equal(s.current_state(), c0) and s.plant_wrench_tick() == 5

    bad = mean.copy(); bad[1, 2] = np.nan
    inf3 = np.array([0.1, np.inf, 0.1])
    cases = [(dict(constant=bad), "brov_current_constant_host: the current must be finite"),
             (dict(table=np.array([[0.1, np.nan, 0.0]])), "brov_current_table_host: table and gain must be finite"),
             (dict(table=np.zeros((2, 3)), gain=[1.0, np.inf, 1.0, 1.0]), "brov_current_table_host: table and gain must be finite"),
             (dict(gauss_markov=dict(gm, mean=bad)), "brov_current_gauss_markov_host: .* must be finite"),
             (dict(gauss_markov=dict(gm, mu=inf3)), "brov_current_gauss_markov_host: .* must be finite"),
             (dict(gauss_markov=dict(gm, amp=[0.1, 0.1, np.nan])), "brov_current_gauss_markov_host: .* must be finite"),
             (dict(gauss_markov=dict(gm, hi=inf3)), "brov_current_gauss_markov_host: .* must be finite"),
             (dict(gauss_markov=dict(gm, step=np.nan)), "brov_current_gauss_markov_host: .* must be finite"),
             (dict(gauss_markov=dict(gm, step=-0.05)), "brov_current_gauss_markov_host: step < 0"),
             (dict(gauss_markov=dict(gm, lo=[-0.3, 0.4, -0.3])), r"brov_current_gauss_markov_host: lo\[i\] > hi\[i\]")]
    for kw, text in cases:
        with pytest.raises(RuntimeError, match=text):
            s.set_current(**kw)
        assert unchanged(), kw
    with pytest.raises(RuntimeError, match="brov_current_set_state_host: the state must be finite"):
        s.set_current_state(bad)
    with pytest.raises(RuntimeError, match="brov_current_eval_host: the Gauss-Markov current is a state"):
        s.current(3)
    # what the Python layer never passes on: null arrays and an empty table
    dp = C.POINTER(C.c_double)
    ok3 = np.zeros((B, 3)).ctypes.data_as(dp)
    L, h = s._L, s._h
    raw = [("brov_current_constant_host", (h, None)), ("brov_current_table_host", (h, None, 2, None)), ("brov_current_table_host", (h, ok3, 0, None)),
           ("brov_current_gauss_markov_host", (h, 5, None, ok3, ok3, None, None, 0.05)), ("brov_current_gauss_markov_host", (h, 5, ok3, None, ok3, None, None, 0.05)),
           ("brov_current_gauss_markov_host", (h, 5, ok3, ok3, None, None, None, 0.05)), ("brov_current_eval_host", (h, 0, None)),
           ("brov_current_get_state_host", (h, None)), ("brov_current_set_state_host", (h, None)), ("brov_current_last_host", (h, None)),
           ("brov_current_last_seconds", (h, None))]
    for name, args in raw:
        assert getattr(L, name)(*args) == -1, name
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())
        assert unchanged(), name
    # the same in a stateless mode: the generator in force stays in force
    tab = rng.uniform(-0.3, 0.3, (5, 3))
    s.set_current(table=tab, gain=[1.0, 2.0, -1.0, 0.5])
    before = s.current(3)
    with pytest.raises(RuntimeError, match="brov_current_eval_host: negative tick"):
        s.current(-1)
    with pytest.raises(RuntimeError, match="brov_current_constant_host"):
        s.set_current(constant=bad)
    assert s.current_mode() == ba.CURRENT_TABLE and np.array_equal(s.current(3), before) and s.plant_wrench_tick() == 5
    with pytest.raises(ValueError):
        s.set_current(table=tab, constant=[0, 0, 0])
    with pytest.raises(ValueError):
        s.set_current(constant=[0, 0, 0], gain=[1, 1, 1, 1])
    with pytest.raises(ValueError):
        s.set_current(gauss_markov=dict(gm, sigma=1.0))
    # the fleet has its own plant kernel, which knows no current
    x0 = np.zeros((B, 12)); x0[:, 2] = -20.0
    s.plant_wrench_seek(0)
    s.set_x0(x0); s.set_candidate_params("circle", np.full(B, 2.0), np.full(B, 0.5), np.zeros(B))
    f = ba.Fleet(s, 2)
    for call in (lambda: f.step(), lambda: f.closed_loop(2, dt_ref=0.05, dt_node=0.05), lambda: f.closed_loop_dob(None, 2, dt_ref=0.05, dt_node=0.05)):
        with pytest.raises(RuntimeError, match="ocean current"):
            call()
    assert np.array_equal(s.get_x0(), x0) and s.plant_wrench_tick() == 0
    s.current_off()
    u, x, st, win = f.closed_loop(2, dt_ref=0.05, dt_node=0.05)
    assert np.isfinite(x).all()
    f.close(); s.close()


def test_a_run_past_tick_2_to_the_22_is_refused_before_any_launch(ba):
    N, B = 20, 8
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    s = _loop_solver(ba, B, N, x0, traj, np.tile(ba.P_NOMINAL, (B, 1)))
    s.set_current(gauss_markov=dict(mean=[0.1, 0.0, 0.0], mu=0.5, amp=0.02))
    e, t = _ekf(ba, B), ba.BatchTrack(B)
    s.plant_wrench_seek(2 ** 22 - 3)
    c = s.current_state()
    for name, call in (("brov_closed_loop", lambda: s.closed_loop(4)), ("brov_closed_loop_dob", lambda: s.closed_loop_dob(e, ticks=4)),
                       ("brov_closed_loop_track", lambda: s.closed_loop_track(t, 4))):
        with pytest.raises(RuntimeError, match=name + r": the Gauss-Markov current .* 2\^22"):
            call()
        assert s.plant_wrench_tick() == 2 ** 22 - 3 and np.array_equal(s.get_x0(), x0) and np.array_equal(s.current_state(), c), name
    log = s.closed_loop(3)                                 # the last three ticks of the counter's range
    assert np.all(log[2] == 0) and s.plant_wrench_tick() == 2 ** 22 and not np.array_equal(s.current_state(), c)
    x3 = s.get_x0()
    with pytest.raises(RuntimeError, match="brov_plant_step: the Gauss-Markov current"):
        s.plant_step(0.05, 1)
    assert np.array_equal(s.get_x0(), x3) and s.plant_wrench_tick() == 2 ** 22
    # a stateless current draws nothing: it runs on
    s.set_current(constant=[0.1, 0.0, 0.0])
    s.plant_step(0.05, 1)
    assert s.plant_wrench_tick() == 2 ** 22 + 1
    e.close(); t.close(); s.close()


# ---- 6. the point of it -------------------------------------------------------------------------------------------------------------------------
def test_the_observer_compensates_a_constant_current(ba):
    """A constant current of 1 m/s at a heading of 0.7 rad on the circle: the DOB loop (the estimate handed to the controller) tracks better
    than the same loop without the hand-off.  Batch 4, 80 ticks, chosen on the CPU loop of tests/current_restatement.py before any GPU run
    (DESIGN.md section 4.9d): RMS position error 0.0941 m with the hand-off against 0.1290 m without, a gap of 27 % (0.8 m/s: 22 %; 0.5 m/s:
    15 %; at 160 ticks the gap halves, the uncompensated loop settling into its offset).  Only the ordering is asserted, and that every step succeeds."""
    N, B, ticks = 20, 4, 80
    rng = np.random.default_rng(21)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
    pp = np.tile(ba.P_NOMINAL, (B, 1))
    vc = ba.current_from_angles(1.0, 0.7, 0.0)
    rms = {}
    for handoff in (True, False):
        s = _loop_solver(ba, B, N, x0, traj, pp); s.set_current(constant=vc)
        e = _ekf(ba, B)
        if handoff:
            log = s.closed_loop_dob(e, ticks=ticks)
            x, st = log["x"], log["status"]
        else:
            _, x, st = s.closed_loop(ticks)
        assert np.all(st == 0) and np.array_equal(s.current_last(), np.tile(vc, (B, 1)))
        err = x[1:, :, :3] - traj[1:ticks + 1, None, :3]
        rms[handoff] = float(np.sqrt((err ** 2).sum(-1).mean()))
        s.close(); e.close()
    print(f"RMS position error in a current of 1 m/s: {rms[True]:.4f} m with the hand-off, {rms[False]:.4f} m without")
    assert rms[True] < rms[False]
