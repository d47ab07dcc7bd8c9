"""GPU tests of the fleet in moving water (brov_vehicle_current_*, brov_vehicle_coriolis_*; fleet_plant_water_kernel in
bluerov2_amd/csrc/fleet_water_kernel.hip): the per-vehicle current generator against tests/current_restatement.py and a plain solver of
batch V, one step against the restated RK4 of tests/coriolis_restatement.py (terms 0: tests/current_restatement.py's), the two `last`
buffers and the force alone, the hold, C = 1 against the solver's own plant, off against the parent path, the loop against its call
sequence, the refusals, and the two scenarios the stages are for.  N = 20 throughout, at most 130 instances."""
import ctypes

import numpy as np
import pytest

import coriolis_restatement as CO
import fleet_restatement as FR
from current_restatement import GM_CASE, CurrentRestatement
from oracle import trajectory_oracle as T
from wrench_restatement import WrenchRestatement

pytestmark = pytest.mark.gpu
N, TS = 20, 0.05
ERR_ARG = -1
PERIODIC = dict(seed=0xC0FFEE123456789, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)
KA, MA = 0.3, 1.2481          # a roll added inertia that is not the reference's zero: the bx q product is exercised
SHAPES = [(5, 3), (130, 1), (1, 1)]


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


def solver(ba, B):
    s = ba.BatchSolver(B, ba.SolverOptions(N, TS))
    s.set_params(ba.P_NOMINAL)
    return s


def _fleet(ba, V, C, seed, tilt=False, plant_params=True):
    """the fleet of tests/test_gpu_fleet_disturbance.py: a solver of batch V * C with circle candidates of distinct radii, distinct start
    states, the vehicles' true parameters (distinct disturbances, damping and -- here -- added masses) unless plant_params=False"""
    B = V * C
    rng = np.random.default_rng(seed)
    s = solver(ba, B)
    s.set_candidate_params("circle", np.tile(2.0 + 0.5 * np.arange(C) / C, V), np.full(B, 0.5), np.zeros(B))
    xv = np.zeros((V, 12)); xv[:, 0] = -2.2; xv[:, 2] = -20.0; xv[:, 5] = -0.5 * np.pi
    xv[:, :3] += rng.normal(size=(V, 3)) * 0.1
    xv[:, 5] += rng.normal(size=V) * 0.05
    if tilt:
        xv[:, 6:] += rng.normal(size=(V, 6)) * 0.1
        xv[:, 3:5] += rng.uniform(-0.4, 0.4, (V, 2))
    pp = np.tile(ba.P_NOMINAL, (V, 1)); pp[:, :4] = rng.uniform(-5, 5, (V, 4)); pp[:, 8:] *= rng.uniform(0.9, 1.1, (V, 8))
    pp[:, 4:7] *= rng.uniform(0.8, 1.2, (V, 3))
    f = ba.Fleet(s, C)
    f.set_state(xv)
    if plant_params:
        f.set_plant_params(pp)
    return s, f, xv, pp


def _ekf(ba, V):
    """the device observer for the device plant, as tests/test_gpu_fleet_disturbance.py configures it"""
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
    return ba.BatchEkf(V, par)


def _gm_mean(V):
    rng = np.random.default_rng(77)
    return rng.uniform(-0.5, 0.6, (V, 3)) * np.array([1.0, 0.5, 0.2])


def _modes(V, rng):
    """(name, Fleet.set_current / BatchSolver.set_current arguments, restatement at batch V) of the three modes; currents of a few tenths
    of a metre per second"""
    vc = rng.uniform(0.1, 0.5, (V, 3)) * rng.choice([-1.0, 1.0], (V, 3))
    tab = rng.uniform(0.1, 0.4, (64, 3)) * rng.choice([-1.0, 1.0], (64, 3))            # tick 140 lies past its end: the last row
    gain = rng.uniform(0.5, 1.5, V)
    mean = _gm_mean(V)
    return [("constant", dict(constant=vc), CurrentRestatement(V).constant(vc)),
            ("table", dict(table=tab, gain=gain), CurrentRestatement(V).table(tab, gain)),
            ("gauss_markov", dict(gauss_markov=dict(mean=mean, **GM_CASE)), CurrentRestatement(V).gauss_markov(mean=mean, **GM_CASE))]


def _set_coriolis(f, terms):
    if terms:
        f.set_coriolis(terms, ka=KA, ma=MA)
    else:
        f.coriolis_off()
    assert f.coriolis_terms() == terms


# ---- 1. the generator per vehicle -------------------------------------------------------------------------------------------------------
def test_generator_is_the_solvers_with_the_vehicle_as_instance(ba):
    V, C = 5, 3
    s, f, xv, _ = _fleet(ba, V, C, seed=1)
    plain = ba.BatchSolver(V, ba.SolverOptions(N, TS))     # a solver of batch V: its instance v is in the current vehicle v is in
    assert f.current_mode() == ba.CURRENT_OFF and not f.current(3).any() and not f.current_state().any()
    for name, kw, r in _modes(V, np.random.default_rng(2)):
        f.set_current(**kw); plain.set_current(**kw)
        assert f.current_mode() == plain.current_mode() == r.mode != ba.CURRENT_OFF
        if name == "gauss_markov":
            for obj in (f, plain):
                with pytest.raises(RuntimeError, match="a state, not a function of the tick"):
                    obj.current(3)
        else:
            for k in (0, 13, 140):
                cf = f.current(k)
                assert cf.shape == (V, 3) and np.abs(cf).max() > 0.05
                assert cf.tobytes() == r.current(k).tobytes(), (name, k)
                assert cf.tobytes() == plain.current(k).tobytes(), (name, k)      # the index is v, not v * C
        st = f.current_state()
        assert st.tobytes() == plain.current_state().tobytes() == r.state(0).tobytes(), name
        assert f.wrench_tick() == 0 and f.state().tobytes() == xv.tobytes()         # evaluation moves neither the counter nor a state
        assert f.current_state().tobytes() == st.tobytes() and not f.current_last().any()
    f.current_off()
    assert f.current_mode() == ba.CURRENT_OFF and not f.current(13).any()
    f.close(); s.close(); plain.close()


def test_gauss_markov_sequence_is_the_restatements_and_does_not_depend_on_c(ba):
    V, tick0 = 5, 1000
    mean = _gm_mean(V)
    seqs = {}
    for C in (3, 1):
        s, f, xv, _ = _fleet(ba, V, C, seed=4)
        s.set_yref_candidates_tick(0.0, TS); s.solve()
        f.set_current(gauss_markov=dict(mean=mean, **GM_CASE)); f.wrench_seek(tick0)
        r = CurrentRestatement(V).gauss_markov(mean=mean, **GM_CASE)
        seq = [f.current_state()]
        assert seq[0].tobytes() == mean.tobytes()
        for k in range(5):
            f.step(None, 0.05, 1)
            applied = r.step(tick0 + k)
            assert f.current_last().tobytes() == applied.tobytes(), (C, k)
            seq.append(f.current_state())
            assert seq[-1].tobytes() == r.c.tobytes(), (C, k)
            assert f.wrench_tick() == tick0 + k + 1
        assert np.abs(seq[-1] - seq[0]).max() > 1e-3
        seqs[C] = np.array(seq)
        f.close(); s.close()
    assert seqs[3].tobytes() == seqs[1].tobytes()


# ---- 2. one step against the restated RK4 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrench", [False, True], ids=["no wrench", "periodic wrench"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["constant", "table", "gauss_markov"])
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("V,C", SHAPES)
def test_step_in_moving_water_matches_the_restated_rk4(ba, oracle, V, C, substeps, mode, wrench):
    s, f, xv, pp = _fleet(ba, V, C, seed=10 * V + C, tilt=True)
    s.set_yref_candidates_tick(0.0, TS); s.solve()
    name, kw, r = _modes(V, np.random.default_rng(3))[mode]
    f.set_current(**kw)
    gen = WrenchRestatement(V).periodic(**PERIODIC)
    c0 = np.where(r.mean >= 0.0, r.mean + 0.2, r.mean - 0.2) if name == "gauss_markov" else None   # a state that is not the mean
    u_ref, worst = None, 0.0
    if wrench:
        f.set_wrench(periodic=PERIODIC)
    for tick in (13, 140):
        w = gen.wrench(tick) if wrench else None
        calm = None
        for terms in (0, 1, 2, 3):
            _set_coriolis(f, terms)
            f.set_state(xv); f.wrench_seek(tick)
            if c0 is not None:
                f.set_current_state(c0); r.set_state(c0)
            f.step(None, 0.05, substeps)
            x1 = f.state()
            u, _, _ = f.last()                              # the input every vehicle was given: the winner's u0
            assert f.wrench_tick() == tick + 1
            vc = r.step(tick)
            assert 0.05 < np.abs(vc).max() < 1.0
            err = np.abs(x1 - CO.plant_step(oracle, xv, u, pp, w, vc, terms, 0.05, substeps, KA, MA)).max()
            worst = max(worst, err)
            assert err < 1e-12, (name, tick, wrench, terms, err)
            if u_ref is None:
                u_ref = u
            assert np.array_equal(u, u_ref)                 # the same u at every step: the records do not change
            if calm is None:                                # the step under the same wrench in still water, without the stage
                calm = CO.plant_step(oracle, xv, u, pp, w, None, 0, 0.05, substeps)
            assert np.abs(x1 - calm).max() > 1e-6, (name, tick, wrench, terms)
            assert s.get_x0().tobytes() == np.repeat(x1, C, axis=0).tobytes()
            assert f.current_last().tobytes() == vc.tobytes()
            if c0 is not None:
                assert f.current_state().tobytes() == r.c.tobytes()
    print(f"V={V} C={C} {name} substeps {substeps}: {'periodic wrench' if wrench else 'no wrench'}: max |x_fleet - x_restated|_inf over 8 steps = {worst:.2e}")
    f.close(); s.close()


# ---- 3. `last` and the force alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant_params", [True, False])
def test_last_buffers_and_the_force_alone(ba, oracle, plant_params):
    V, C, tick = 5, 3, 13
    s, f, xv, pp = _fleet(ba, V, C, seed=6, tilt=True, plant_params=plant_params)
    if not plant_params:
        pp = np.tile(ba.P_NOMINAL, (V, 1))                      # what the fleet's plant reads without them: stage 0 of candidate 0
    s.set_yref_candidates_tick(0.0, TS); s.solve()
    rng = np.random.default_rng(8)
    x = rng.normal(size=(V, 12)) * 0.5
    vcs = rng.uniform(-0.5, 0.5, (V, 3))
    assert not f.coriolis_eval(x, vcs).any()                    # off: zeros
    for name, kw, r in _modes(V, np.random.default_rng(9)):
        for terms in (1, 2, 3):
            f.set_current(**kw); _set_coriolis(f, terms)
            assert not f.current_last().any() and not f.coriolis_last().any(), (name, terms)      # zeros before the first step
            assert f.coriolis_eval(x, vcs).tobytes() == CO.force_at(terms, x, pp, vcs, KA, MA).tobytes()
            assert f.coriolis_eval(x).tobytes() == CO.force_at(terms, x, pp, None, KA, MA).tobytes()
            assert f.coriolis_eval(x, vcs[0]).tobytes() == CO.force_at(terms, x, pp, np.tile(vcs[0], (V, 1)), KA, MA).tobytes()
            f.set_state(xv); f.wrench_seek(tick)
            f.step(None, 0.05, 1)
            vc = r.step(tick)
            assert f.current_last().tobytes() == vc.tobytes(), (name, terms)
            want = CO.force_at(terms, xv, pp, vc, KA, MA)
            assert np.abs(want).max() > 1e-3
            assert f.coriolis_last().tobytes() == want.tobytes(), (name, terms)
            if not plant_params:                                # the strided read of the controller's stage-0 parameters
                u, _, _ = f.last()
                assert np.abs(f.state() - CO.plant_step(oracle, xv, u, pp, None, vc, terms, 0.05, 1, KA, MA)).max() < 1e-12
            f.reset()
            assert not f.current_last().any() and not f.coriolis_last().any(), (name, terms)      # ... and after reset()
            assert f.wrench_tick() == 0 and f.current_mode() == r.mode and f.coriolis_terms() == terms   # modes and settings stay
            if name == "gauss_markov":
                assert f.current_state().tobytes() == r.mean.tobytes()                              # the state back at its mean
                r.set_state(r.mean)
    # the stage in still water: the current's `last` is left alone, the force is that of x[6..9) itself
    f.current_off(); _set_coriolis(f, 3)
    f.set_state(xv)
    f.step(None, 0.05, 1)
    assert f.coriolis_last().tobytes() == CO.force_at(3, xv, pp, None, KA, MA).tobytes() and not f.current_last().any()
    u, _, _ = f.last()
    assert np.abs(f.state() - CO.plant_step(oracle, xv, u, pp, None, None, 3, 0.05, 1, KA, MA)).max() < 1e-12
    f.close(); s.close()


# ---- 4. the hold is unchanged under water -----------------------------------------------------------------------------------------------
def _synthetic_records(V, C, seed):
    rng = np.random.default_rng(seed)
    B = V * C
    r = np.zeros(B, dtype=FR.RESULT_DTYPE)
    r["u0"] = rng.uniform(-20, 20, (B, 4)); r["cost"] = rng.normal(size=B) * 10; r["kkt"] = rng.uniform(0, 5, B)
    return r


def _device_records(r):
    import torch
    return torch.from_numpy(np.frombuffer(r.tobytes(), dtype=np.uint8).copy()).cuda()


def test_hold_in_moving_water(ba, oracle):
    import torch
    V = C = 3
    r1 = _synthetic_records(V, C, seed=1)
    r2 = _synthetic_records(V, C, seed=2)
    r2f = r2.copy(); r2f["status"][C:2 * C] = [4, 2, 3]             # vehicle 1: no eligible candidate
    gen = WrenchRestatement(V).periodic(**PERIODIC)
    vc = np.random.default_rng(12).uniform(-0.5, 0.5, (V, 3))
    runs = {}
    for name, second in (("fail", r2f), ("ok", r2)):
        s, f, xv, pp = _fleet(ba, V, C, seed=5, tilt=True)
        f.set_wrench(periodic=PERIODIC); f.wrench_seek(13)
        f.set_current(constant=vc); _set_coriolis(f, 3)
        d1, d2 = _device_records(r1), _device_records(second)
        f.step(d1.data_ptr(), 0.05, 1)
        u1, st1, w1 = f.last()
        x1 = f.state()
        f.step(d2.data_ptr(), 0.05, 1)
        u2, st2, w2 = f.last()
        ew, eu, es = FR.apply(second, V, C, u1)
        assert np.array_equal(w2, ew) and np.array_equal(u2, eu) and np.array_equal(st2, es)        # the status rule is unchanged
        assert f.wrench_tick() == 15
        x2 = f.state()
        err = np.abs(x2 - CO.plant_step(oracle, x1, u2, pp, gen.wrench(14), vc, 3, 0.05, 1, KA, MA)).max()
        print(f"[hold in moving water, {name}] |x_fleet - x_restated|_inf = {err:.2e}")
        assert err < 1e-12
        if name == "fail":
            assert w2[1] == -1 and st2[1] == 4 and np.array_equal(u2[1], u1[1])                      # held input, candidate 0's status
            held = CO.plant_step(oracle, x1[1:2], u1[1:2], pp[1:2], gen.wrench(14)[1:2], vc[1:2], 3, 0.05, 1, KA, MA)
            assert np.abs(x2[1] - held[0]).max() < 1e-12
        runs[name] = (x2, s.get_x0(), u2, f.coriolis_last())
        torch.cuda.synchronize()
        f.close(); s.close()
    for v in (0, 2):                                                # vehicles 0 and 2 do not see vehicle 1's failure
        assert runs["fail"][0][v].tobytes() == runs["ok"][0][v].tobytes()
        assert runs["fail"][1][v * C:(v + 1) * C].tobytes() == runs["ok"][1][v * C:(v + 1) * C].tobytes()
        assert runs["fail"][3][v].tobytes() == runs["ok"][3][v].tobytes()
    assert runs["fail"][0][1].tobytes() != runs["ok"][0][1].tobytes()


# ---- 5. C = 1 is the solver's plant, tick by tick ---------------------------------------------------------------------------------------
def test_one_candidate_per_vehicle_is_the_solvers_plant_tick_by_tick(ba):
    V, ticks, tick0, t0 = 130, 3, 20, 0.3
    a, f, xv, pp = _fleet(ba, V, 1, seed=7)
    mean = _gm_mean(V)
    gm = dict(gauss_markov=dict(mean=mean, **GM_CASE))
    f.set_wrench(periodic=PERIODIC); f.wrench_seek(tick0)
    f.set_current(**gm); _set_coriolis(f, 3)
    b = solver(ba, V)                                               # the twin: the fleet's state goes in at every tick
    b.set_candidate_params("circle", np.full(V, 2.0), np.full(V, 0.5), np.zeros(V))
    b.set_plant_params(pp); b.set_plant_wrench(periodic=PERIODIC)
    b.set_current(**gm); b.set_coriolis(rigid=True, added=True, ka=KA, ma=MA)
    assert b.current_state().tobytes() == f.current_state().tobytes() == mean.tobytes()
    worst, same, x = 0.0, True, xv
    for k in range(ticks):
        a.set_yref_candidates_tick(t0 + k * TS, TS); a.solve()
        wk = f.wrench(tick0 + k)
        f.step(None, 0.05, 2)
        uf, stf, winf = f.last()
        xf = f.state()
        b.set_x0(x)
        b.set_yref_candidates_tick(t0 + k * TS, TS); b.solve()
        res = b.results()
        b.plant_wrench_seek(tick0 + k)
        assert b.plant_wrench(tick0 + k).tobytes() == wk.tobytes() and np.abs(wk).max() > 1.0
        b.plant_step(0.05, 2)
        xb = b.get_x0()
        assert res["u0"].tobytes() == uf.tobytes() and np.array_equal(res["status"], stf), k
        assert np.array_equal(winf, np.where(res["status"] == 0, 0, -1))
        worst = max(worst, np.abs(xb - xf).max())
        same = same and xb.tobytes() == xf.tobytes()
        assert b.current_state().tobytes() == f.current_state().tobytes(), k        # the Gauss-Markov states, after every tick
        assert b.current_last().tobytes() == f.current_last().tobytes() and b.coriolis_last().tobytes() == f.coriolis_last().tobytes(), k
        x = xf
    print(f"[fleet C=1 in a Gauss-Markov current, terms 3, periodic wrench] max |x_fleet - x_plant_step| = {worst:.3e}, bit-identical: {same}")
    assert worst < 1e-12
    assert np.abs(f.current_state() - mean).max() > 1e-3
    f.close(); a.close(); b.close()


# ---- 6. off is the parent path ----------------------------------------------------------------------------------------------------------
def test_off_is_the_parent_path_and_a_zero_current_agrees_with_it(ba):
    V, C, ticks = 5, 3, 4
    logs = {}
    for name in ("parent", "off", "zero"):
        s, f, xv, pp = _fleet(ba, V, C, seed=8)
        if name == "off":
            for _, kw, _ in _modes(V, np.random.default_rng(1)):
                f.set_current(**kw)
            f.set_coriolis(3, ka=KA, ma=MA)
            f.current_off(); f.coriolis_off()
        if name == "zero":
            f.set_current(constant=np.zeros(3))
        assert f.current_mode() == (ba.CURRENT_CONSTANT if name == "zero" else ba.CURRENT_OFF) and f.coriolis_terms() == 0
        logs[name] = f.closed_loop(ticks, t0=0.0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=2) + (f.state(), s.get_x0())
        assert f.wrench_tick() == ticks
        f.close(); s.close()
    for p, q in zip(logs["parent"], logs["off"]):
        assert p.tobytes() == q.tobytes()
    (up, xp, sp, wp, _, _), (uz, xz, sz, wz, _, _) = logs["parent"], logs["zero"]
    print(f"zero current against the parent path: |du| = {np.abs(up - uz).max():.2e}, |dx| = {np.abs(xp - xz).max():.2e}, "
          f"bit-identical: {xp.tobytes() == xz.tobytes()}")
    assert np.array_equal(sp, sz) and np.array_equal(wp, wz) and np.abs(up - uz).max() < 1e-12 and np.abs(xp - xz).max() < 1e-12


# ---- 7. the loop equals its call sequence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("observer", [True, False])
def test_closed_loop_dob_equals_its_call_sequence_in_moving_water(ba, observer):
    V, C, ticks, tick0, t0 = 5, 3, 6, 20, 0.1
    rng = np.random.default_rng(31)
    tab = rng.uniform(-0.4, 0.4, (16, 3)); gain = rng.uniform(0.5, 1.5, V)     # one body of water, V vehicles; the table ends inside the run
    out = []
    for fused in (True, False):
        s, f, xv, pp = _fleet(ba, V, C, seed=10 * V + C)
        f.set_current(table=tab, gain=gain); _set_coriolis(f, 1); f.wrench_seek(tick0 - 8)
        e = _ekf(ba, V) if observer else None
        if fused:
            log = f.closed_loop_dob(e, ticks + 8, t0=t0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=2)
            log = {k: v for k, v in log.items() if v is not None}
        else:
            log = dict(u=[], x=[f.state()], status=[], winner=[], wrench=[], est=[])
            for k in range(ticks + 8):
                s.set_yref_candidates_tick(t0 + k * TS, TS); s.solve()
                log["wrench"].append(f.wrench(f.wrench_tick()))
                f.step(None, 0.05, 2)
                if observer:
                    f.observe(e, 0.05)
                    f.apply_estimate(e)
                    log["est"].append(e.state()[0][:, 12:].copy())
                u, st, win = f.last()
                log["u"].append(u); log["status"].append(st); log["winner"].append(win); log["x"].append(f.state())
            if not observer:
                del log["est"]
            log = {k: np.array(v) for k, v in log.items()}
        out.append((log, s.get_params(), s.get_x0(), e.state() if observer else None, f.state(), f.wrench_tick(), f.current_last(),
                    f.coriolis_last()))
        f.close(); s.close()
        if observer:
            e.close()
    (la, pa, xa, ea, fa, ta, ca, ka), (lb, pb, xb, eb, fb, tb, cb, kb) = out
    assert set(la) == set(lb)
    for key in la:
        assert la[key].dtype == lb[key].dtype and la[key].tobytes() == lb[key].tobytes(), key
    assert pa.tobytes() == pb.tobytes() and xa.tobytes() == xb.tobytes() and fa.tobytes() == fb.tobytes()
    assert ca.tobytes() == cb.tobytes() == (tab[-1][None, :] * gain[:, None]).tobytes() and ka.tobytes() == kb.tobytes()
    if observer:
        assert ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
        assert np.abs(pa[:, :, :4]).max() > 0.01                  # the hand-off reached the controller's parameters
    assert ta == tb == tick0 + ticks
    assert np.all(la["status"] == 0) and not la["wrench"].any()
    assert xa.tobytes() == np.repeat(fa, C, axis=0).tobytes()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(ba):
    from bluerov2_amd.fleet import _fleet_lib
    L = _fleet_lib()
    V, C = 2, 3
    s, f, xv, pp = _fleet(ba, V, C, seed=3)
    h = f._h
    x0 = s.get_x0()
    mean = _gm_mean(V)
    dp = ctypes.POINTER(ctypes.c_double)
    P = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)   # noqa: E731
    err = lambda: L.brov_fleet_last_error().decode()   # noqa: E731
    three, nan3 = np.full(3, 0.1), np.array([0.1, np.nan, 0.1])
    v3 = np.full((V, 3), 0.2); bad3 = v3.copy(); bad3[1, 2] = np.inf
    out3 = np.full((V, 3), 7.0); out4 = np.full((V, 4), 7.0); x12 = np.zeros((V, 12))
    t, ka, ma = ctypes.c_int(-1), ctypes.c_double(-1.0), ctypes.c_double(-1.0)

    def state_of_things():
        assert L.brov_vehicle_coriolis_get(h, ctypes.byref(t), ctypes.byref(ka), ctypes.byref(ma)) == 0
        return (f.current_mode(), f.coriolis_terms(), t.value, ka.value, ma.value, f.wrench_tick(), f.state().tobytes(), s.get_x0().tobytes(),
                f.current_state().tobytes())

    assert L.brov_vehicle_coriolis_get(h, ctypes.byref(t), ctypes.byref(ka), ctypes.byref(ma)) == 0 and (t.value, ka.value, ma.value) == (0, 0.0, 1.2481)
    f.set_current(gauss_markov=dict(mean=mean, **GM_CASE)); f.set_coriolis(2, ka=0.25, ma=0.75); f.wrench_seek(5)
    before = state_of_things()
    assert before[:6] == (ba.CURRENT_GAUSS_MARKOV, 2, 2, 0.25, 0.75, 5)
    gm_ok = (h, 1, P(mean), P(three), P(three), None, None, 0.05)
    cases = [
        ("brov_vehicle_current_constant_host", (h, None), "null argument"),
        ("brov_vehicle_current_constant_host", (h, P(bad3)), "the current must be finite"),
        ("brov_vehicle_current_table_host", (h, None, 2, None), "needs a table and rows >= 1"),
        ("brov_vehicle_current_table_host", (h, P(v3), 0, None), "needs a table and rows >= 1"),
        ("brov_vehicle_current_table_host", (h, P(bad3), V, None), "table and gain must be finite"),
        ("brov_vehicle_current_table_host", (h, P(v3), V, P([1.0, np.nan])), "table and gain must be finite"),
        ("brov_vehicle_current_gauss_markov_host", (h, 1, None, P(three), P(three), None, None, 0.05), "null argument"),
        ("brov_vehicle_current_gauss_markov_host", (h, 1, P(mean), None, P(three), None, None, 0.05), "null argument"),
        ("brov_vehicle_current_gauss_markov_host", (h, 1, P(mean), P(three), None, None, None, 0.05), "null argument"),
        ("brov_vehicle_current_gauss_markov_host", (h, 1, P(bad3), P(three), P(three), None, None, 0.05), "mean, mu, amp, lo, hi and step must be finite"),
        ("brov_vehicle_current_gauss_markov_host", (h, 1, P(mean), P(nan3), P(three), None, None, 0.05), "mean, mu, amp, lo, hi and step must be finite"),
        ("brov_vehicle_current_gauss_markov_host", (h, 1, P(mean), P(three), P(nan3), None, None, 0.05), "mean, mu, amp, lo, hi and step must be finite"),
        ("brov_vehicle_current_gauss_markov_host", (h, 1, P(mean), P(three), P(three), P(nan3), None, 0.05), "mean, mu, amp, lo, hi and step must be finite"),
        ("brov_vehicle_current_gauss_markov_host", (h, 1, P(mean), P(three), P(three), None, P(nan3), 0.05), "mean, mu, amp, lo, hi and step must be finite"),
        ("brov_vehicle_current_gauss_markov_host", gm_ok[:7] + (np.nan,), "mean, mu, amp, lo, hi and step must be finite"),
        ("brov_vehicle_current_gauss_markov_host", gm_ok[:7] + (-0.05,), "step < 0"),
        ("brov_vehicle_current_gauss_markov_host", (h, 1, P(mean), P(three), P(three), P([0.0, 0.3, 0.0]), P([0.1, 0.2, 0.1]), 0.05), "lo[i] > hi[i]"),
        ("brov_vehicle_current_gauss_markov_host", (h, 1, P(mean), P(three), P(three), P([6.0, 0.0, 0.0]), None, 0.05), "lo[i] > hi[i]"),
        ("brov_vehicle_current_eval_host", (h, 3, None), "null argument"),
        ("brov_vehicle_current_eval_host", (h, -1, P(out3)), "negative tick"),
        ("brov_vehicle_current_eval_host", (h, 3, P(out3)), "the Gauss-Markov current is a state, not a function of the tick"),
        ("brov_vehicle_current_get_state_host", (h, None), "null argument"),
        ("brov_vehicle_current_set_state_host", (h, None), "null argument"),
        ("brov_vehicle_current_set_state_host", (h, P(bad3)), "the state must be finite"),
        ("brov_vehicle_current_last_host", (h, None), "null argument"),
        ("brov_vehicle_coriolis_set", (h, 0, 0.0, 1.0), "terms must be"), ("brov_vehicle_coriolis_set", (h, 4, 0.0, 1.0), "terms must be"),
        ("brov_vehicle_coriolis_set", (h, -1, 0.0, 1.0), "terms must be"),
        ("brov_vehicle_coriolis_set", (h, 1, np.nan, 1.0), "ka and ma must be finite and not negative"),
        ("brov_vehicle_coriolis_set", (h, 1, -0.1, 1.0), "ka and ma"), ("brov_vehicle_coriolis_set", (h, 1, np.inf, 1.0), "ka and ma"),
        ("brov_vehicle_coriolis_set", (h, 3, 0.0, np.nan), "ka and ma"), ("brov_vehicle_coriolis_set", (h, 3, 0.0, -1.0), "ka and ma"),
        ("brov_vehicle_coriolis_get", (h, None, ctypes.byref(ka), ctypes.byref(ma)), "null argument"),
        ("brov_vehicle_coriolis_get", (h, ctypes.byref(t), None, ctypes.byref(ma)), "null argument"),
        ("brov_vehicle_coriolis_get", (h, ctypes.byref(t), ctypes.byref(ka), None), "null argument"),
        ("brov_vehicle_coriolis_eval_host", (h, None, None, P(out4)), "null argument"),
        ("brov_vehicle_coriolis_eval_host", (h, P(x12), None, None), "null argument"),
        ("brov_vehicle_coriolis_last_host", (h, None), "null argument"),
    ]
    for name, args, text in cases:
        assert getattr(L, name)(*args) == ERR_ARG, (name, args)
        assert err().startswith(name + ": " + text), (name, err())
        assert state_of_things() == before, name
        assert np.all(out3 == 7.0) and np.all(out4 == 7.0), name
    # only the Gauss-Markov current has a state to set
    f.set_current(constant=v3)
    assert L.brov_vehicle_current_set_state_host(h, P(v3)) == ERR_ARG
    assert err().startswith("brov_vehicle_current_set_state_host: only the Gauss-Markov current has a state")
    assert f.current_mode() == ba.CURRENT_CONSTANT and f.current(3).tobytes() == v3.tobytes()
    with pytest.raises(RuntimeError, match="brov_vehicle_coriolis_set: terms must be"):
        f.set_coriolis(0)
    # the 2^22 limit of the Gauss-Markov counter: asked before anything is enqueued
    f.set_current(gauss_markov=dict(mean=mean, **GM_CASE)); f.set_current_state(mean + 0.01)
    f.wrench_seek(2 ** 22 - 1)
    s.set_yref_candidates_tick(0.0, TS); s.solve()
    before = state_of_things()
    for loop in (lambda: f.closed_loop(2, dt_ref=TS, dt_node=TS), lambda: f.closed_loop_dob(None, 2, dt_ref=TS, dt_node=TS)):
        with pytest.raises(RuntimeError, match=r"brov_closed_loop_fleet(_dob)?: the Gauss-Markov current draws at the plant's tick, which must stay below 2\^22"):
            loop()
        assert state_of_things() == before
    assert L.brov_fleet_step(h, None, 0.05, 1, None) == 0           # the step at the last tick runs ...
    assert f.wrench_tick() == 2 ** 22 and f.current_state().tobytes() != before[8]
    after = state_of_things()
    assert L.brov_fleet_step(h, None, 0.05, 1, None) == ERR_ARG     # ... the next one would draw at 2^22
    assert err().startswith("brov_fleet_step: the Gauss-Markov current draws at the plant's tick") and state_of_things() == after
    f.current_off()
    assert L.brov_fleet_step(h, None, 0.05, 1, None) == 0           # without the Gauss-Markov mode the counter is free
    # the SOLVER's own current and Coriolis stage are indexed by the instance: the fleet calls refuse them as before
    f.reset(); f.set_state(xv); f.set_current(constant=v3)
    calls = (("brov_fleet_step", lambda: f.step()), ("brov_closed_loop_fleet", lambda: f.closed_loop(2, dt_ref=TS, dt_node=TS)),
             ("brov_closed_loop_fleet_dob", lambda: f.closed_loop_dob(None, 2, dt_ref=TS, dt_node=TS)))
    s.set_current(constant=[0.1, 0.0, 0.0])
    for name, call in calls:
        with pytest.raises(RuntimeError, match=name + r": an ocean current of the solver's plant is in force \(brov_current_\*\); the fleet's plant "
                                                      r"integrates the vehicles in still water"):
            call()
    s.current_off(); s.set_coriolis(rigid=True)
    for name, call in calls:
        with pytest.raises(RuntimeError, match=name + r": the Coriolis stage of the solver's plant is on \(brov_coriolis_set\); the fleet's plant "
                                                      r"integrates the OCP model, which has no such forces"):
            call()
    assert np.array_equal(s.get_x0(), x0) and f.wrench_tick() == 0 and f.state().tobytes() == xv.tobytes()
    s.coriolis_off()
    u, x, st, win = f.closed_loop(2, dt_ref=TS, dt_node=TS)
    assert np.isfinite(x).all() and f.wrench_tick() == 2 and f.current_last().tobytes() == v3.tobytes()
    f.close(); s.close()


# ---- 9. what it is for ------------------------------------------------------------------------------------------------------------------
def _scenario(ba, V, C, ticks, seed=21):
    rng = np.random.default_rng(seed)
    ref = T.candidate_windows("circle", ticks, [2.0], [1.5], [0.0], 0.0, TS)[0]      # row k: the candidates' reference at t = k * TS
    xv = np.zeros((V, 12)); xv[:, :6] = ref[0, :6]; xv[:, :3] += rng.normal(size=(V, 3)) * 0.05
    return ref, xv


def _scenario_fleet(ba, V, C, xv):
    s = solver(ba, V * C)
    s.set_candidate_params("circle", np.full(V * C, 2.0), np.full(V * C, 1.5), np.zeros(V * C))
    f = ba.Fleet(s, C)
    f.set_state(xv); f.set_plant_params(np.tile(ba.P_NOMINAL, (V, 1)))
    return s, f


def test_the_observers_hand_off_helps_in_a_current(ba):
    """Four vehicles x four candidates (all the same circle, r = 2 m, v = 1.5 m/s: candidate 0 always wins) in ONE constant horizontal current
    of 0.5 m/s, 80 ticks of brov_closed_loop_fleet_dob: RMS position error with the observer's hand-off, without it, and in still water
    with it.  The orderings are asserted, the values printed (DESIGN.md section 4.12c has them)."""
    V, C, ticks = 4, 4, 80
    ref, xv = _scenario(ba, V, C, ticks)
    vc = np.array([0.5 * np.cos(0.6), 0.5 * np.sin(0.6), 0.0])
    rms = {}
    for name, current, handoff in (("handoff", True, True), ("none", True, False), ("still", False, True)):
        s, f = _scenario_fleet(ba, V, C, xv)
        if current:
            f.set_current(constant=vc)
        e = _ekf(ba, V)
        log = f.closed_loop_dob(e if handoff else None, ticks, t0=0.0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1)
        assert np.all(log["status"] == 0) and not log["winner"].any()
        assert f.current_last().tobytes() == (np.tile(vc, (V, 1)) if current else np.zeros((V, 3))).tobytes()
        err = log["x"][1:, :, :3] - ref[1:ticks + 1, None, :3]
        rms[name] = float(np.sqrt((err ** 2).sum(-1).mean()))
        f.close(); s.close(); e.close()
    print(f"RMS position error in a 0.5 m/s current: {rms['handoff']:.4f} m with the hand-off, {rms['none']:.4f} m without; "
          f"still water with the hand-off: {rms['still']:.4f} m")
    assert rms["handoff"] < rms["none"]
    assert rms["still"] < rms["none"]


def test_the_phantom_force_goes_with_the_rigid_body_terms_on_the_fleets_plant(ba):
    """Still water, no wrench, the observer on, 4 x 4, 80 ticks: the observer's model has the rigid-body Coriolis products, the fleet's bare
    plant does not, and the estimate carries the difference as a force nobody applies.  With CORIOLIS_RIGID on the fleet's plant the median
    |estimate| of the x and y disturbances over the last 20 ticks is smaller.  Orderings asserted, values printed."""
    V, C, ticks = 4, 4, 80
    ref, xv = _scenario(ba, V, C, ticks)
    med = {}
    for terms in (0, ba.CORIOLIS_RIGID):
        s, f = _scenario_fleet(ba, V, C, xv)
        if terms:
            f.set_coriolis(terms)                                    # the reference's coefficients: ka = 0, ma = 1.2481
        e = _ekf(ba, V)
        log = f.closed_loop_dob(e, ticks, t0=0.0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1)
        assert np.all(log["status"] == 0) and np.isfinite(log["x"]).all() and not log["wrench"].any()
        med[terms] = CO.phantom_medians(log["est"])
        f.close(); s.close(); e.close()
    off, rigid = med[0], med[ba.CORIOLIS_RIGID]
    print(f"median |estimate| over the last 20 ticks: X {off[0]:.4f} N, Y {off[1]:.4f} N on the bare plant; "
          f"X {rigid[0]:.4f} N, Y {rigid[1]:.4f} N with CORIOLIS_RIGID on the fleet's plant")
    assert rigid[0] < off[0]
    assert rigid[1] < off[1]
