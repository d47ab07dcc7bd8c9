"""GPU tests of the fleet under disturbance (brov_vehicle_*, brov_closed_loop_fleet_dob; fleet_plant_wrench_kernel,
fleet_observe_inputs_kernel, fleet_apply_kernel in bluerov2_amd/csrc/fleet_kernel.hip): the per-vehicle wrench generator against
tests/wrench_restatement.py and against a plain solver of batch V, one step against the restated RK4, the hold under a wrench, the loop
against the solver's own wrench plant and against its own call sequence, the observer hand-off in isolation, and the argument checks.
N = 20 throughout, at most 130 instances."""
import ctypes
import math
import os

import numpy as np
import pytest

import fleet_restatement as FR
from oracle import trajectory_oracle as T
from wrench_restatement import WrenchRestatement, plant_step

pytestmark = pytest.mark.gpu
N, TS = 20, 0.05
ERR_ARG = -1
ROTOR = 0.026546960744430276
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrench_tables.npz")
PERIODIC = dict(seed=0xC0FFEE123456789, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)


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


def _modes(V, rng):
    """(name, setter arguments, restatement at batch V) of the three modes, magnitudes as in tests/test_gpu_plant_wrench.py"""
    tab = np.load(GOLDEN)["table"]
    wc = rng.uniform(-100, 100, (V, 6)); wc[:, 3:] *= 0.05
    gain = rng.uniform(-5, 5, V)
    return [("constant", dict(constant=wc), WrenchRestatement(V).constant(wc)),
            ("periodic", dict(periodic=PERIODIC), WrenchRestatement(V).periodic(**PERIODIC)),
            ("table", dict(table=tab, gain=gain), WrenchRestatement(V).table(tab, gain))]


def _fleet(ba, V, C, seed, tilt=False, plant_params=True):
    """a solver of batch V * C with circle candidates of distinct radii, a fleet over it at distinct start states, the vehicles' true
    parameters (distinct disturbances and damping) unless plant_params=False"""
    B = V * C
    rng = np.random.default_rng(seed)
    s = solver(ba, B)
    s.set_candidate_params("circle", np.tile(2.0 + 0.5 * np.arange(C) / C, V), np.full(B, 0.5), np.zeros(B))
    xv = np.zeros((V, 12)); xv[:, 0] = -2.2; xv[:, 2] = -20.0; xv[:, 5] = -0.5 * np.pi
    xv[:, :3] += rng.normal(size=(V, 3)) * 0.1
    xv[:, 5] += rng.normal(size=V) * 0.05
    if tilt:
        xv[:, 6:] += rng.normal(size=(V, 6)) * 0.1
        xv[:, 3:5] += rng.uniform(-0.4, 0.4, (V, 2))      # roll and pitch of a few tenths of a radian: the projection matters
    pp = np.tile(ba.P_NOMINAL, (V, 1)); pp[:, :4] = rng.uniform(-5, 5, (V, 4)); pp[:, 8:] *= rng.uniform(0.9, 1.1, (V, 8))
    f = ba.Fleet(s, C)
    f.set_state(xv)
    if plant_params:
        f.set_plant_params(pp)
    return s, f, xv, pp


def _ekf(ba, V):
    """the device observer for the device plant: the OCP model itself, unit scaling, no roll / pitch thrust (brov_ekf_apply_to_solver in
    include/bluerov2_nmpc.h; the helper of tests/test_gpu_plant_wrench.py restated)"""
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
    return ba.BatchEkf(V, par)


def _allocation(u):
    """the thrust vector fleet_observe_inputs_kernel writes, operation for operation"""
    inv = 1.0 / ROTOR
    return np.stack([(-u[:, 0] + u[:, 1] + u[:, 3]) * inv, (-u[:, 0] - u[:, 1] - u[:, 3]) * inv, (u[:, 0] + u[:, 1] - u[:, 3]) * inv,
                     (u[:, 0] - u[:, 1] + u[:, 3]) * inv, (-u[:, 2]) * inv, (-u[:, 2]) * inv], axis=1)


# ---- 1. the generator per vehicle -------------------------------------------------------------------------------------------------------
def test_generator_is_the_solvers_with_the_vehicle_as_instance(ba):
    V, C = 5, 3
    s, f, xv, _ = _fleet(ba, V, C, seed=1)
    plain = ba.BatchSolver(V, ba.SolverOptions(N, TS))     # a solver of batch V: its instance v draws what vehicle v draws
    assert f.wrench_mode() == ba.WRENCH_OFF and not f.wrench(3).any()
    for name, kw, r in _modes(V, np.random.default_rng(2)):
        f.set_wrench(**kw); plain.set_plant_wrench(**kw)
        assert f.wrench_mode() == plain.plant_wrench_mode() != ba.WRENCH_OFF
        for k in (0, 13, 140):
            wf, wr = f.wrench(k), r.wrench(k)
            assert wf.shape == (V, 6)
            if name == "periodic":
                np.testing.assert_allclose(wf, wr, rtol=1e-14, atol=0, err_msg=f"tick {k}")
            else:
                assert np.array_equal(wf, wr), (name, k)
            assert wf.tobytes() == plain.plant_wrench(k).tobytes(), (name, k)      # the index is v, not v * C
        assert f.wrench_tick() == 0 and f.state().tobytes() == xv.tobytes()         # evaluation moves nothing
    f.wrench_off()
    assert f.wrench_mode() == ba.WRENCH_OFF and not f.wrench(13).any()
    f.close(); s.close(); plain.close()


# ---- 2. one step against the restated RK4 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 4])
@pytest.mark.parametrize("V,C", [(5, 3), (130, 1), (1, 1)])
def test_step_under_a_wrench_matches_the_restated_rk4(ba, oracle, V, C, substeps):
    s, f, xv, pp = _fleet(ba, V, C, seed=10 * V + C, tilt=True)
    s.set_yref_candidates_tick(0.0, TS); s.solve()
    calm = None
    for name, kw, r in _modes(V, np.random.default_rng(3)):
        f.set_wrench(**kw)
        for tick in (13, 140):
            f.set_state(xv); f.wrench_seek(tick)
            f.step(None, 0.05, substeps)
            x1 = f.state()
            u, _, _ = f.last()                                  # the input every vehicle was given: the winner's u0 (or the held one)
            assert f.wrench_tick() == tick + 1
            w = r.wrench(tick)
            assert 1.0 < np.abs(w).max() < 300.0
            err = np.abs(x1 - plant_step(oracle, xv, u, pp, w, 0.05, substeps)).max()
            print(f"V={V} C={C} {name} tick {tick} substeps {substeps}: |x_fleet - x_restated|_inf = {err:.2e}")
            assert err < 1e-12, (name, tick, err)
            # ... and the wrench is felt: the step without it lands elsewhere (the same u at every step: the records do not change)
            if calm is None:
                calm = (u, plant_step(oracle, xv, u, pp, np.zeros((V, 6)), 0.05, substeps))
            assert np.array_equal(u, calm[0])
            assert np.abs(x1 - calm[1]).max() > 1e-6
            assert s.get_x0().tobytes() == np.repeat(x1, C, axis=0).tobytes()
    f.close(); s.close()


# ---- 3. the hold under a wrench ---------------------------------------------------------------------------------------------------------
def _synthetic_records(V, C, seed):
    rng = np.random.default_rng(seed)
    B = V * C
    r = np.zeros(B, dtype=FR.RESULT_DTYPE)
    r["u0"] = rng.uniform(-20, 20, (B, 4)); r["cost"] = rng.normal(size=B) * 10; r["kkt"] = rng.uniform(0, 5, B)
    return r


def _device_records(r):
    import torch
    return torch.from_numpy(np.frombuffer(r.tobytes(), dtype=np.uint8).copy()).cuda()


def test_hold_under_a_wrench(ba, oracle):
    V = C = 3
    r1 = _synthetic_records(V, C, seed=1)
    r2 = _synthetic_records(V, C, seed=2)
    r2f = r2.copy(); r2f["status"][C:2 * C] = [4, 2, 3]             # vehicle 1: no eligible candidate
    gen = WrenchRestatement(V).periodic(**PERIODIC)
    runs = {}
    for name, second in (("fail", r2f), ("ok", r2)):
        s, f, xv, pp = _fleet(ba, V, C, seed=5, tilt=True)
        f.set_wrench(periodic=PERIODIC); f.wrench_seek(13)
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
        err = np.abs(x2 - plant_step(oracle, x1, u2, pp, gen.wrench(14), 0.05, 1)).max()
        print(f"[hold under a wrench, {name}] |x_fleet - x_restated|_inf = {err:.2e}")
        assert err < 1e-12
        if name == "fail":
            assert w2[1] == -1 and st2[1] == 4 and np.array_equal(u2[1], u1[1])                      # held input, candidate 0's status
            held = plant_step(oracle, x1[1:2], u1[1:2], pp[1:2], gen.wrench(14)[1:2], 0.05, 1)
            assert np.abs(x2[1] - held[0]).max() < 1e-12
        runs[name] = (x2, s.get_x0(), u2)
        import torch
        torch.cuda.synchronize()
        f.close(); s.close()
    for v in (0, 2):                                                # vehicles 0 and 2 do not see vehicle 1's failure
        assert runs["fail"][0][v].tobytes() == runs["ok"][0][v].tobytes()
        assert runs["fail"][1][v * C:(v + 1) * C].tobytes() == runs["ok"][1][v * C:(v + 1) * C].tobytes()
    assert runs["fail"][0][1].tobytes() != runs["ok"][0][1].tobytes()


# ---- 4. C = 1 against the solver's own wrench plant -------------------------------------------------------------------------------------
def test_one_candidate_per_vehicle_is_the_solvers_wrench_plant_step_by_step(ba):
    V, ticks, tick0, t0 = 130, 3, 20, 0.3
    a, f, xv, pp = _fleet(ba, V, 1, seed=7)
    f.set_wrench(periodic=PERIODIC); f.wrench_seek(tick0)
    log = f.closed_loop_dob(None, ticks, t0=t0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=2)
    assert log["est"] is None and np.array_equal(log["x"][0], xv) and f.wrench_tick() == tick0 + ticks
    b = solver(ba, V)                                               # the twin: the fleet's state goes in at every tick
    b.set_candidate_params("circle", np.full(V, 2.0), np.full(V, 0.5), np.zeros(V))
    b.set_plant_params(pp); b.set_plant_wrench(periodic=PERIODIC)
    worst, same = 0.0, True
    for k in range(ticks):
        b.set_x0(log["x"][k])
        b.set_yref_candidates_tick(t0 + k * TS, TS); b.solve()
        res = b.results()
        b.plant_wrench_seek(tick0 + k)
        assert b.plant_wrench(tick0 + k).tobytes() == log["wrench"][k].tobytes()
        b.plant_step(0.05, 2)
        x = b.get_x0()
        assert np.array_equal(res["u0"], log["u"][k]) and np.array_equal(res["status"], log["status"][k]), k
        assert np.array_equal(log["winner"][k], np.where(res["status"] == 0, 0, -1))
        worst = max(worst, np.abs(x - log["x"][k + 1]).max())
        same = same and x.tobytes() == log["x"][k + 1].tobytes()
    print(f"[fleet C=1 under the periodic wrench] max |x_fleet - x_plant_step| = {worst:.3e}, bit-identical: {same}")
    assert worst < 1e-12
    assert np.abs(log["wrench"]).max() > 1.0
    f.close(); a.close(); b.close()


# ---- 5. mode OFF is the parent path -----------------------------------------------------------------------------------------------------
def test_mode_off_is_the_parent_path_and_a_zero_wrench_agrees_with_it(ba):
    V, C, ticks = 5, 3, 4
    logs = {}
    for name in ("parent", "off", "zero"):
        s, f, xv, pp = _fleet(ba, V, C, seed=8)
        if name == "off":
            f.set_wrench(constant=np.random.default_rng(1).uniform(-50, 50, (V, 6))); f.set_wrench(periodic=PERIODIC); f.wrench_off()
        if name == "zero":
            f.set_wrench(constant=np.zeros(6))
        assert f.wrench_mode() == (ba.WRENCH_CONSTANT if name == "zero" else ba.WRENCH_OFF)
        logs[name] = f.closed_loop(ticks, t0=0.0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=2) + (f.state(), s.get_x0())
        assert f.wrench_tick() == ticks
        f.close(); s.close()
    for p, q in zip(logs["parent"], logs["off"]):
        assert p.tobytes() == q.tobytes()
    (up, xp, sp, wp, _, _), (uz, xz, sz, wz, _, _) = logs["parent"], logs["zero"]
    print(f"zero wrench against the parent path: |du| = {np.abs(up - uz).max():.2e}, |dx| = {np.abs(xp - xz).max():.2e}")
    assert np.array_equal(sp, sz) and np.abs(up - uz).max() < 1e-12 and np.abs(xp - xz).max() < 1e-12


# ---- 6. the hand-off in isolation -------------------------------------------------------------------------------------------------------
def test_observe_and_apply_estimate_in_isolation(ba):
    V, C = 5, 3
    s, f, xv, pp = _fleet(ba, V, C, seed=9)
    f.set_wrench(periodic=PERIODIC); f.wrench_seek(20)
    e, twin = _ekf(ba, V), _ekf(ba, V)
    vprev = np.zeros((V, 6))
    for k in range(2):                                              # the second round meets velocities kept from the first
        s.set_yref_candidates_tick(k * TS, TS); s.solve()
        f.step(None, 0.05, 1)
        x = f.state()
        u, _, _ = f.last()
        f.observe(e, 0.05)
        twin.update(_allocation(u), x, (x[:, 6:] - vprev) / 0.05)
        vprev = x[:, 6:].copy()
        (xe, Pe), (xt, Pt) = e.state(), twin.state()
        assert xe.tobytes() == xt.tobytes() and Pe.tobytes() == Pt.tobytes(), k
    before = s.get_params()
    f.apply_estimate(e)
    after = s.get_params()
    mp = e.outputs()[1]
    assert np.abs(mp).max() > 0.0
    assert np.array_equal(after[:, :, :4], np.broadcast_to(np.repeat(mp, C, axis=0)[:, None, :], (V * C, N + 1, 4)))
    assert after[:, :, 4:].tobytes() == np.ascontiguousarray(before[:, :, 4:]).tobytes()
    # reset forgets the velocities: the next observation sees (v - 0) / dt again
    f.reset(); f.set_state(x)
    f.observe(e, 0.05)
    twin.update(_allocation(np.zeros((V, 4))), x, x[:, 6:] / 0.05)
    assert e.state()[0].tobytes() == twin.state()[0].tobytes()
    f.close(); s.close(); e.close(); twin.close()


# ---- 7. the loop equals its call sequence -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,C", [(5, 3), (2, 65)])
def test_closed_loop_dob_equals_its_call_sequence(ba, V, C):
    ticks, tick0, t0 = 6, 20, 0.1
    out = []
    for fused in (True, False):
        s, f, xv, pp = _fleet(ba, V, C, seed=10 * V + C)
        f.set_wrench(periodic=PERIODIC); f.wrench_seek(tick0)
        e = _ekf(ba, V)
        if fused:
            log = f.closed_loop_dob(e, ticks, t0=t0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=2)
        else:
            log = dict(u=[], x=[f.state()], status=[], winner=[], wrench=[], est=[])
            for k in range(ticks):
                s.set_yref_candidates_tick(t0 + k * TS, TS); s.solve()
                log["wrench"].append(f.wrench(f.wrench_tick()))
                f.step(None, 0.05, 2)
                f.observe(e, 0.05)
                f.apply_estimate(e)
                u, st, win = f.last()
                log["u"].append(u); log["status"].append(st); log["winner"].append(win); log["x"].append(f.state())
                log["est"].append(e.state()[0][:, 12:].copy())
            log = {k: np.array(v) for k, v in log.items()}
        out.append((log, s.get_params(), s.get_x0(), e.state(), f.state(), f.wrench_tick()))
        f.close(); s.close(); e.close()
    (la, pa, xa, ea, fa, ta), (lb, pb, xb, eb, fb, tb) = out
    for key in ("u", "x", "status", "winner", "wrench", "est"):
        assert la[key].dtype == lb[key].dtype and la[key].tobytes() == lb[key].tobytes(), key
    assert pa.tobytes() == pb.tobytes() and xa.tobytes() == xb.tobytes() and fa.tobytes() == fb.tobytes()
    assert ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes()
    assert ta == tb == tick0 + ticks
    print(f"[loop V={V} C={C}] |wrench|max = {np.abs(la['wrench']).max():.3f}, |p[..., :4]|max = {np.abs(pa[:, :, :4]).max():.3f}, "
          f"winners {la['winner'].tolist()}")
    assert np.all(la["status"] == 0) and np.abs(la["wrench"]).max() > 1.0
    assert np.abs(pa[:, :, :4]).max() > 0.1                   # the hand-off reached the controller's parameters
    assert xa.tobytes() == np.repeat(fa, C, axis=0).tobytes()


def test_closed_loop_dob_without_an_observer_is_closed_loop_under_the_wrench(ba):
    V, C, ticks = 5, 3, 6
    runs = {}
    for name, wrench, dob in (("dob", True, True), ("loop", True, False), ("dob off", False, True), ("loop off", False, False)):
        s, f, xv, pp = _fleet(ba, V, C, seed=53)
        if wrench:
            f.set_wrench(periodic=PERIODIC); f.wrench_seek(20)
        if dob:
            log = f.closed_loop_dob(None, ticks, t0=0.1, dt_ref=TS, dt_node=TS, dt=0.05, substeps=2)
            assert log["est"] is None and (np.abs(log["wrench"]).max() > 1.0 if wrench else not log["wrench"].any())
            runs[name] = (log["u"], log["x"], log["status"], log["winner"])
        else:
            runs[name] = f.closed_loop(ticks, t0=0.1, dt_ref=TS, dt_node=TS, dt=0.05, substeps=2)
        f.close(); s.close()
    for p, q in (("dob", "loop"), ("dob off", "loop off")):
        for x, y in zip(runs[p], runs[q]):
            assert x.tobytes() == y.tobytes(), (p, q)
    assert runs["dob"][1].tobytes() != runs["loop off"][1].tobytes()      # a twin whose wrench is OFF agrees only when the fleet's is OFF too


# ---- 8. compensation helps --------------------------------------------------------------------------------------------------------------
def test_compensation_helps_under_the_reference_constant_world_wrench(ba):
    """The reference's mode 1, (10, 10, 10, 0, 0, 0) N in the world frame, on a fleet of V = 4 vehicles x C = 2 candidates, both
    candidates of a vehicle the same circle (r = 2 m, v = 1.5 m/s: candidate 0 always wins), 80 ticks: the loop with the observer's
    hand-off tracks better than the loop without it.  Checked on the CPU before any GPU run with wrench_restatement.cpu_dob_loop on a
    table cut from the candidates' generator (oracle.trajectory_oracle.candidate_windows), same start states: RMS position error
    0.0913 m with the hand-off against 0.0996 m without.  Only the ordering is asserted here, and that every step succeeds."""
    V, C, ticks = 4, 2, 80
    rng = np.random.default_rng(21)
    ref = T.candidate_windows("circle", ticks, [2.0], [1.5], [0.0], 0.0, TS)[0]      # row k: the candidates' reference at t = k * TS
    xv = np.zeros((V, 12)); xv[:, :6] = ref[0, :6]; xv[:, :3] += rng.normal(size=(V, 3)) * 0.05
    rms = {}
    for handoff in (True, False):
        s = solver(ba, V * C)
        s.set_candidate_params("circle", np.full(V * C, 2.0), np.full(V * C, 1.5), np.zeros(V * C))
        f = ba.Fleet(s, C)
        f.set_state(xv); f.set_plant_params(np.tile(ba.P_NOMINAL, (V, 1)))
        f.set_wrench(constant=[10, 10, 10, 0, 0, 0])
        e = _ekf(ba, V)
        log = f.closed_loop_dob(e if handoff else None, ticks, t0=0.0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1)
        assert np.all(log["status"] == 0) and not log["winner"].any()
        assert np.array_equal(log["wrench"], np.broadcast_to([10.0, 10, 10, 0, 0, 0], (ticks, V, 6)))
        err = log["x"][1:, :, :3] - ref[1:ticks + 1, None, :3]
        rms[handoff] = float(np.sqrt((err ** 2).sum(-1).mean()))
        f.close(); s.close(); e.close()
    print(f"RMS position error under (10, 10, 10) N: {rms[True]:.4f} m compensated, {rms[False]:.4f} m uncompensated")
    assert rms[True] < rms[False]


# ---- 9. arguments -----------------------------------------------------------------------------------------------------------------------
def test_arguments(ba):
    from bluerov2_amd.fleet import _fleet_lib
    L = _fleet_lib()
    V, C = 2, 3
    s, f, xv, pp = _fleet(ba, V, C, seed=3, plant_params=False)
    x0 = s.get_x0()
    e, wrong = _ekf(ba, V), _ekf(ba, V + 1)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    u = np.full((2, V, 4), 7.0); x = np.full((3, V, 12), 7.0); st = np.full((2, V), 7, dtype=np.int32); win = np.full((2, V), 7, dtype=np.int32)
    w = np.full((2, V, 6), 7.0); est = np.full((2, V, 6), 7.0)
    logs = (u.ctypes.data_as(dp), x.ctypes.data_as(dp), st.ctypes.data_as(ip), win.ctypes.data_as(ip), w.ctypes.data_as(dp))
    loop = lambda eh, ticks, est_p: L.brov_closed_loop_fleet_dob(f._h, eh, ticks, 0.0, TS, TS, 0.05, 1, *logs, est_p)   # noqa: E731

    def refused(rc):
        assert rc == ERR_ARG and L.brov_fleet_last_error().decode()
        assert np.array_equal(s.get_x0(), x0)
        assert np.all(u == 7.0) and np.all(x == 7.0) and np.all(st == 7) and np.all(win == 7) and np.all(w == 7.0) and np.all(est == 7.0)

    # the fleet's plant parameters unset: the estimate would be fed back into the plant
    refused(L.brov_vehicle_apply_estimate(f._h, e._h, None))
    assert "brov_fleet_set_plant_params_host" in L.brov_fleet_last_error().decode()
    refused(loop(e._h, 2, est.ctypes.data_as(dp)))
    with pytest.raises(RuntimeError):
        f.apply_estimate(e)
    with pytest.raises(RuntimeError):
        f.closed_loop_dob(e, 2)
    f.set_plant_params(pp)
    # an observer whose batch is not V
    refused(L.brov_vehicle_observe(f._h, wrong._h, 0.05, None))
    refused(L.brov_vehicle_apply_estimate(f._h, wrong._h, None))
    refused(loop(wrong._h, 2, est.ctypes.data_as(dp)))
    refused(L.brov_vehicle_observe(f._h, e._h, 0.0, None))
    # an estimate log without an observer
    refused(loop(None, 2, est.ctypes.data_as(dp)))
    # the generator's arguments
    refused(L.brov_vehicle_wrench_periodic(f._h, 1, 6.0, 0.0, 0.125, 0.0))          # tz_div = 0
    refused(L.brov_vehicle_wrench_table_host(f._h, w.ctypes.data_as(dp), 0, None))  # rows < 1
    refused(L.brov_vehicle_wrench_seek(f._h, -1))
    assert f.wrench_mode() == ba.WRENCH_OFF and f.wrench_tick() == 0
    f.set_wrench(periodic=dict(dphi=1.0))
    edge = int(2 ** 22 * math.pi)                                   # the last tick whose half-period index has 22 bits
    refused(L.brov_vehicle_wrench_seek(f._h, edge + 8))
    refused(L.brov_vehicle_wrench_eval_host(f._h, edge + 8, w.ctypes.data_as(dp)))
    f.wrench_seek(edge - 1)                                         # ticks edge - 1 and edge are in range, the third is not
    refused(loop(e._h, 3, est.ctypes.data_as(dp)))
    refused(loop(None, 3, None))
    assert f.wrench_tick() == edge - 1
    f.wrench_seek(edge)
    assert L.brov_fleet_step(f._h, None, 0.05, 1, None) == 0        # the step at the edge runs, the next one would leave the range
    refused_after = L.brov_fleet_step(f._h, None, 0.05, 1, None)
    assert refused_after == ERR_ARG and L.brov_fleet_last_error().decode() and f.wrench_tick() == edge + 1
    f.wrench_off(); f.wrench_seek(0); f.set_state(xv)
    # the solver's own wrench mode and the 6-disturbance variant are still refused
    s.set_plant_wrench(constant=[10, 10, 10, 0, 0, 0])
    refused(loop(e._h, 2, est.ctypes.data_as(dp)))
    refused(L.brov_fleet_step(f._h, None, 0.05, 1, None))
    s.plant_wrench_off()
    s.enable_dist6(True)
    refused(loop(e._h, 2, est.ctypes.data_as(dp)))
    refused(L.brov_fleet_step(f._h, None, 0.05, 1, None))
    refused(L.brov_vehicle_apply_estimate(f._h, e._h, None))
    s.enable_dist6(False)
    refused(loop(e._h, -1, est.ctypes.data_as(dp)))
    # ... and with valid arguments the same loop runs
    f.set_wrench(periodic=PERIODIC)
    assert loop(e._h, 2, est.ctypes.data_as(dp)) == 0
    assert np.array_equal(x[0], xv) and not any(np.any(a == 7.0) for a in (u, x, w, est)) and np.all(win >= -1) and np.all(win < C)
    assert f.wrench_tick() == 2 and np.array_equal(w[1], f.wrench(1))
    f.close(); s.close(); e.close(); wrong.close()
