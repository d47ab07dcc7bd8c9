"""GPU tests of the plant's delay stage (brov_delay_*, delay_shift_kernel, delay_predict_kernel) against tests/delay_restatement.py, the
oracle's model / RTI step / EKF, and the call sequences the loops replace.  N = 20 throughout."""
import numpy as np
import pytest

from oracle import trajectory_oracle as T
from oracle.oracle_ffi import EkfOracle
from delay_restatement import DelayRestatement, cpu_delay_loop, rms_position_error
from thruster_restatement import ThrusterRestatement

pytestmark = pytest.mark.gpu
N = 20
SCENARIOS = (("none", 0, 0), ("delayed", 2, 0), ("predicted", 2, 2))   # name, delay, comp: the columns of DESIGN.md section 4.9e's table


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


def _start(ba, B, seed=21, spread=None):
    """(trajectory, start states near its first row, true plant parameters), left unchanged.  Seed 21 without `spread` is the setup of
    DESIGN.md section 4.9e: N(0, 0.05) on the position alone"""
    rng = np.random.default_rng(seed)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    if spread is None:
        x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
    else:
        x0 += rng.normal(size=(B, 12)) * spread
    pp = np.tile(ba.P_NOMINAL, (B, 1))
    for a in (traj, x0, pp):
        a.setflags(write=False)
    return traj, x0, pp


def _loop_solver(ba, B, x0, traj, pp):
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(pp); s.set_trajectory(traj)
    return s


def _ekf_pair(ba, B):
    """device observer and oracle EKF for the device plant, as tests/test_gpu_thrusters.py::_ekf_pair configures them"""
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    orc = EkfOracle(); orc.par.compensate_coef = 1.0; orc.par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
        orc.par.K[j] = 0.0
    return (ba.BatchEkf(B, par) if B else None), orc


@pytest.fixture(scope="module")
def cpu_scenarios(ba, oracle):
    """the three CPU loops of the table over 40 ticks, computed once: name -> (log, RMS position error)"""
    traj, x0, pp = _start(ba, 4)
    out = {}
    for name, delay, comp in SCENARIOS:
        log = cpu_delay_loop(oracle, DelayRestatement(4, delay, comp), traj, x0, ba.P_NOMINAL, pp, N, 40)
        out[name] = (log, rms_position_error(log["x"], traj))
    return out


# ---- 1. identity -------------------------------------------------------------------------------------------------------------------------
def test_no_delay_and_no_prediction_is_the_parent_loop(ba):
    B, ticks = 130, 12                                               # one full block plus two lanes
    traj, x0, _ = _start(ba, B, 3, np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3))
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = np.random.default_rng(4).uniform(-60, 60, (B, 4))
    off, on = _loop_solver(ba, B, x0, traj, pp), _loop_solver(ba, B, x0, traj, pp)
    on.set_delay()                                                   # all delays 0, comp 0
    assert on.delay_enabled() and not off.delay_enabled() and on.delay_comp() == 0 and on.delay_depth() == 1
    la, lb = off.closed_loop(ticks, line0=2), on.closed_loop(ticks, line0=2)
    for name, a, b in zip(("u", "x", "status"), la, lb):
        assert np.array_equal(a, b), name
    assert off.results().tobytes() == on.results().tobytes() and np.array_equal(off.get_x0(), on.get_x0())
    assert off.plant_wrench_tick() == on.plant_wrench_tick() == ticks
    au, at = on.delay_last()                                         # what was applied is what was commanded
    assert np.array_equal(au, on.results()["u0"]) and np.array_equal(at, on.results()["thrust"])
    shift_s, predict_s = on.delay_last_seconds()
    assert 0.0 < shift_s < 1.0 and predict_s is None                 # comp 0: the predictor was never launched
    # stage off again: the one-launch loop is back
    on.delay_off(); on.set_x0(x0); on.init_iterate_default()
    off.set_x0(x0); off.init_iterate_default()
    for a, b in zip(off.closed_loop(ticks, line0=2), on.closed_loop(ticks, line0=2)):
        assert np.array_equal(a, b)
    on.solve_ticks(1, row_stride=1, sync=True)                       # (the window in force names rows of the table: the one-launch form left it)
    off.close(); on.close()


# ---- 2. the queue, bit for bit -------------------------------------------------------------------------------------------------------------
def test_queue_matches_the_restatement_bit_for_bit(ba, oracle):
    B, ticks, line0 = 130, 9, 1                                      # D = 4: the ring wraps twice
    delay = np.arange(B) % 4
    traj, x0, _ = _start(ba, B, 5, np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3))
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = np.random.default_rng(6).uniform(-60, 60, (B, 4))
    s = _loop_solver(ba, B, x0, traj, pp)
    s.set_delay(delay)
    assert s.delay_depth() == 4 and s.delay_comp() == 0
    r = DelayRestatement(B, delay)
    assert not s.delay_queue().any() and not s.delay_last()[0].any()
    s.plant_wrench_seek(1000)                                        # the ring is indexed by the stage's own step count, not by this counter
    cmd, xs, worst = [], [s.get_x0()], 0.0
    for k in range(ticks):
        s.set_yref_from_trajectory(line0 + k, 16); s.solve()
        res = s.results()
        x_prev = s.get_x0()
        s.plant_step(0.05, 1)
        au, at = r.step(res["u0"], res["thrust"])
        gu, gt = s.delay_last()
        assert np.array_equal(gu, au) and np.array_equal(gt, at), k
        assert np.array_equal(s.delay_queue(), r.queue()), k
        x1 = s.get_x0()
        ref = np.stack([oracle.rk4(x_prev[b], au[b], pp[b], 0.05) for b in range(B)])
        worst = max(worst, float(np.abs(x1 - ref).max()))
        assert np.array_equal(s.results()["u0"], res["u0"])           # the solver's own records stay the commanded ones
        cmd.append(res["u0"].copy()); xs.append(x1)
    print(f"plant step with the applied input against oracle.rk4, worst of {ticks} steps: {worst:.2e}")
    assert worst < 1e-12                                             # the single-step bound of test_plant_step_matches_oracle_rk4
    cmd = np.array(cmd)
    last_u = s.delay_last()[0]                                       # instances of delay 1: step 8 applied the command of step 7, not its own
    assert np.array_equal(last_u[1::4], cmd[7, 1::4]) and not np.array_equal(last_u[1::4], cmd[8, 1::4])
    assert s.plant_wrench_tick() == 1000 + ticks
    # the `u` log of the loop holds the COMMANDED inputs: the same run through brov_closed_loop
    b = _loop_solver(ba, B, x0, traj, pp); b.set_delay(delay)
    ul, xl, sl = b.closed_loop(ticks, line0=line0)
    assert np.array_equal(ul, cmd) and np.array_equal(xl, np.array(xs)) and not sl.any()
    assert np.array_equal(b.delay_queue(), r.queue()) and np.array_equal(b.delay_last()[0], r.last[:, :4])
    # reset: zeros again, and the first applied records of the delayed instances are zeros again
    b.delay_reset()
    assert not b.delay_queue().any() and not b.delay_last()[0].any()
    b.plant_step(0.05, 1)
    assert not b.delay_last()[0][delay > 0].any() and np.array_equal(b.delay_last()[0][delay == 0], b.results()["u0"][delay == 0])
    s.close(); b.close()


# ---- 3. the predictor ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comp,dist6,dt_pred", [(1, False, None), (1, True, None), (3, False, 0.04), (3, True, 0.04)])
def test_predictor_matches_chained_oracle_rk4(ba, oracle, comp, dist6, dt_pred):
    B = 130
    rng = np.random.default_rng(10 * comp + dist6)
    traj, x0, pp = _start(ba, B, 7, np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3))
    # per-instance parameters whose stage-0 row differs from every other stage's: the predictor must read stage 0
    p = np.tile(ba.P_NOMINAL, (B, N + 1, 1)); p[:, :, :4] = rng.uniform(-5, 5, (B, N + 1, 4)); p[:, 0, :4] = rng.uniform(-40, 40, (B, 4))
    p[:, 0, 4:] *= rng.uniform(0.9, 1.1, (B, 12))
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(p); s.set_plant_params(pp); s.set_trajectory(traj)
    drp = None
    if dist6:
        s.enable_dist6()
        d = rng.uniform(-0.5, 0.5, (B, N + 1, 2)); d[:, 0] = rng.uniform(-3, 3, (B, 2))
        s.set_rp_disturbance(d)
        drp = d[:, 0]
    s.set_delay(np.arange(B) % 3, comp=comp, dt_pred=dt_pred)
    assert s.delay_comp() == comp and s.delay_depth() == max(2, comp) + 1
    r = DelayRestatement(B, np.arange(B) % 3, comp)
    h = 0.05 if dt_pred is None else dt_pred                           # SolverOptions(20): Ts = 1 / 20
    y = x0 + rng.normal(size=(B, 12)) * 0.05
    for steps in range(3):                                             # the queue empty, then one and two commanded records in it
        if steps:
            s.set_yref_from_trajectory(steps + comp, 16); s.solve()
            res = s.results()
            s.plant_step(0.05, 1)
            r.step(res["u0"], res["thrust"])
        assert np.array_equal(s.delay_queue(), r.queue())
        ref = r.predict(oracle, y, p[:, 0], h, drp)
        got = s.delay_predict(y)
        err = float(np.abs(got - ref).max())
        print(f"comp {comp}, dist6 {dist6}, {steps} records in the queue: |x^_gpu - x^_oracle|_inf = {err:.2e}")
        assert err <= comp * 1e-12, (steps, err)
        assert np.abs(got - y).max() > 1e-4                            # the predictor moved the state
        if comp > steps:
            assert not r.predictor_inputs()[0].any()                   # (a slot never written: the zero input)
    # without a state of its own the predictor starts from the controller's; the next solve starts from exactly that
    xc = s.get_x0()
    mine = s.delay_predict()
    assert np.array_equal(mine, s.delay_predict(xc))
    before = (s.delay_queue(), s.get_x0(), s.results().tobytes())
    assert np.array_equal(before[0], r.queue())                        # (the predictor alone moved nothing)
    s.set_yref_from_trajectory(3 + comp, 16); s.solve()
    assert np.array_equal(s.delay_predicted(), mine)
    assert np.abs(mine - r.predict(oracle, xc, p[:, 0], h, drp)).max() <= comp * 1e-12
    assert 0.0 < s.delay_last_seconds()[1] < 1.0
    s.close()


def test_predictor_start_states_and_refusals(ba):
    B = 6
    traj, x0, pp = _start(ba, B, 9, 0.03)
    # comp = 0 leaves the solve's x0 the controller's state: the records of a solver with the stage on are those of one without
    a, b = _loop_solver(ba, B, x0, traj, pp), _loop_solver(ba, B, x0, traj, pp)
    a.set_delay(np.arange(B) % 4, comp=0)
    for s in (a, b):
        s.set_yref_from_trajectory(0, 16); s.solve()
    assert a.results().tobytes() == b.results().tobytes()
    with pytest.raises(RuntimeError, match="brov_delay_predicted_host: no solve has run the predictor"):
        a.delay_predicted()
    assert np.array_equal(a.delay_predict(), a.get_x0())               # comp 0: the predictor is the identity
    b.close()
    # comp = 2: a different initial state, hence different records
    a.set_delay(np.arange(B) % 4, comp=2)
    a.set_yref_from_trajectory(2, 16); a.solve(); a.plant_step(0.05, 1)
    # sensor stage on: the predictor starts from the measured state
    a.set_sensors(seed=11, sigma=np.full((B, 12), 0.01), bias=np.full((B, 12), 0.02))
    ym, xt = a.measured_state(), a.get_x0()
    assert np.abs(ym - xt).max() > 1e-3
    assert np.array_equal(a.delay_predict(), a.delay_predict(ym)) and not np.array_equal(a.delay_predict(), a.delay_predict(xt))
    want = a.delay_predict(ym)
    a.set_yref_from_trajectory(3, 16); a.solve()
    assert np.array_equal(a.delay_predicted(), want)
    # a tick that brings its own x0 is refused while comp > 0; one without is solved from the prediction
    before = (a.results().tobytes(), a.get_x0())
    with pytest.raises(RuntimeError, match="brov_tick_host: the delay stage predicts"):
        a.tick(x0=xt)
    assert a.results().tobytes() == before[0] and np.array_equal(a.get_x0(), before[1])
    rec = a.tick(yref=traj[4:4 + N + 1])
    assert rec.tobytes() == a.results().tobytes() and np.array_equal(a.delay_predicted(), want)   # (neither plant nor queue moved in between)
    a.set_delay(np.arange(B) % 4, comp=0)
    a.tick(x0=xt)                                                      # comp 0: the caller's measurement, as ever
    # arguments: refused, and nothing changes
    a.set_delay(np.arange(B) % 4, comp=2, dt_pred=0.04)
    for kw, text in ((dict(delay=[0, 1, 2, 3, 4, 9]), r"brov_delay_set_host: delay must lie in \[0, BROV_DELAY_MAX\]"),
                     (dict(delay=[0, 1, 2, -1, 0, 0]), "brov_delay_set_host: delay must lie"), (dict(comp=9), "brov_delay_set_host: comp must lie"),
                     (dict(comp=-1), "brov_delay_set_host: comp must lie"), (dict(dt_pred=np.nan), "brov_delay_set_host: dt_pred must be finite"),
                     (dict(dt_pred=np.inf), "brov_delay_set_host: dt_pred must be finite")):
        with pytest.raises(RuntimeError, match=text):
            a.set_delay(**kw)
        assert a.delay_enabled() and a.delay_comp() == 2 and a.delay_depth() == 4
    a.close()


# ---- 4. composition with the other stages; the fleet -------------------------------------------------------------------------------------------
def test_thruster_stage_sees_the_delayed_thrusts_and_the_fleet_refuses_the_stage(ba):
    B, ticks = 6, 5
    traj, x0, pp = _start(ba, B, 13, 0.03)
    s = _loop_solver(ba, B, x0, traj, pp)
    gain = np.ones((B, 6)); gain[:, 0] = 0.0                           # thruster 0 dead
    s.set_plant_wrench(constant=[10.0, 10.0, 10.0, 0.0, 0.0, 0.0])
    s.set_thrusters(lo=-100.0, hi=100.0, gain=gain)
    s.set_delay(2)
    rd, rt = DelayRestatement(B, 2), ThrusterRestatement(B, None, -100.0, 100.0, gain)
    for k in range(ticks):
        s.set_yref_from_trajectory(k, 16); s.solve()
        res = s.results()
        tick = s.plant_wrench_tick()
        s.plant_step(0.05, 1)
        _, at = rd.step(res["u0"], res["thrust"])
        a, _ = rt.step(tick, at)                                       # the stage's restatement on the DELAYED thrusts
        assert np.array_equal(s.thruster_last(), a), k
        assert np.array_equal(s.delay_last()[1], at), k
        if k < 2:
            assert not a.any()
    st = s.thruster_stats()
    assert np.array_equal(st["clip_ticks"], rt.clip_ticks) and np.array_equal(st["lost_sq"], rt.lost_sq) and st["steps"] == ticks
    assert np.abs(s.thruster_last()).max() > 1.0
    s.close()
    # the fleet has its own plant kernel, which knows no delay
    Bf = 4
    f_s = ba.BatchSolver(Bf, ba.SolverOptions(10, 0.05))
    f_s.set_params(ba.P_NOMINAL)
    xf = np.zeros((Bf, 12)); xf[:, 2] = -20.0
    f_s.set_x0(xf); f_s.set_candidate_params("circle", np.full(Bf, 2.0), np.full(Bf, 0.5), np.zeros(Bf))
    f_s.set_delay(1)
    f = ba.Fleet(f_s, 2)
    for call in (lambda: f.step(), lambda: f.closed_loop(2, dt_ref=0.05, dt_node=0.05), lambda: f.closed_loop_dob(None, 2, dt_ref=0.05, dt_node=0.05)):
        with pytest.raises(RuntimeError, match=r"failed \(-1\): brov_.*: the delay stage"):   # BROV_ERR_ARG under the call's name
            call()
    f_s.delay_off()
    f.step()
    f.close(); f_s.close()


# ---- 5. the point of it --------------------------------------------------------------------------------------------------------------------------
def test_prediction_repairs_most_of_what_a_two_tick_delay_costs_on_the_device(ba, cpu_scenarios):
    """The setup of DESIGN.md section 4.9e's table on the device: B = 4, 40 ticks (never longer: the uncompensated loop turns non-finite at
    tick 92 on the CPU).  The ordering the CPU test asserts, and the RMS values against the CPU loop's to the tolerance
    tests/test_gpu_thrusters.py::test_dob_loop_behind_the_stage_agrees_with_the_cpu_loop uses for states."""
    B, ticks = 4, 40
    traj, x0, pp = _start(ba, B)
    rms = {}
    for name, delay, comp in SCENARIOS:
        s = _loop_solver(ba, B, x0, traj, pp)
        if delay or comp:
            s.set_delay(delay, comp=comp)
        ul, xl, sl = s.closed_loop(ticks)
        assert np.isfinite(xl).all() and np.isfinite(ul).all(), name
        assert not sl.any() and not cpu_scenarios[name][0]["status"].any(), name
        rms[name] = rms_position_error(xl, traj)
        print(f"{name}: RMS position error {rms[name]:.6f} m on the device, {cpu_scenarios[name][1]:.6f} m on the CPU; "
              f"|dx| = {np.abs(xl - cpu_scenarios[name][0]['x']).max():.2e}")
        s.close()
    assert rms["predicted"] < 0.5 * rms["delayed"]
    assert rms["predicted"] < 2.0 * rms["none"]
    for name in rms:
        np.testing.assert_allclose(rms[name], cpu_scenarios[name][1], rtol=1e-6, atol=1e-6, err_msg=name)


# ---- 6. what the observer is fed -----------------------------------------------------------------------------------------------------------------
def test_observer_fed_the_applied_thrusts_agrees_with_the_cpu_loop(ba, oracle):
    """Delay 2 with observer_applied: 20 ticks of the device DOB loop against the CPU loop whose EKF is fed the applied thrusts, with the
    tolerances of tests/test_gpu_thrusters.py::test_dob_loop_behind_the_stage_agrees_with_the_cpu_loop; without the flag the estimate differs."""
    B, ticks = 4, 20
    traj, x0, pp = _start(ba, B)
    _, eo = _ekf_pair(ba, 0)
    cpu = cpu_delay_loop(oracle, DelayRestatement(B, 2), traj, x0, ba.P_NOMINAL, pp, N, ticks, ekf=eo, observer_applied=True)
    est = {}
    for flag in (True, False):
        s = _loop_solver(ba, B, x0, traj, pp); s.set_delay(2, observer_applied=flag)
        e, _ = _ekf_pair(ba, B)
        log = s.closed_loop_dob(e, ticks=ticks)
        est[flag] = log["est"]
        bad = np.nonzero(log["status"].any(axis=1))[0]
        print(f"observer_applied {flag}: first tick with a failed step: {bad[0] if len(bad) else None}")
        if flag:
            assert np.all(log["status"] == 0) and np.all(cpu["status"] == 0)
            mp_gpu = s.get_params()[:, 0, :4]
            gx, ge, gp = np.abs(log["x"] - cpu["x"]).max(), np.abs(log["est"] - cpu["est"]).max(), np.abs(mp_gpu - cpu["mpc_p"][-1]).max()
            print(f"GPU loop against CPU loop over {ticks} ticks: |dx| = {gx:.2e}, |d est| = {ge:.2e}, |d mpc_p| = {gp:.2e}")
            assert np.abs(log["u"] - cpu["applied_u"]).max() > 1e-3     # the u log holds the commanded input: tick 0 applied zeros
            np.testing.assert_allclose(log["x"], cpu["x"], rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(log["est"], cpu["est"], rtol=1e-5, atol=1e-4)
            np.testing.assert_allclose(mp_gpu, cpu["mpc_p"][-1], rtol=1e-5, atol=5e-3)
        s.close(); e.close()
    # (fed the commanded thrusts the observer charges the missing thrust to a disturbance, and handing that to a controller that is two ticks
    # late need not end well: only tick 0 is compared, where the plant was given zeros and the observer was told so or not)
    d0 = np.abs(est[True][0] - est[False][0]).max()
    print(f"estimate after tick 0 with the applied thrusts against the commanded ones: |d est| = {d0:.2e}")
    assert np.isfinite(est[False][0]).all() and d0 > 0.0 and not np.array_equal(est[True], est[False])


# ---- 7. the loops agree --------------------------------------------------------------------------------------------------------------------------
def test_scored_loop_in_chunks_equals_the_tracker_fed_with_the_logged_loop(ba):
    B, ticks, line0 = 6, 12, 1
    traj, x0, pp = _start(ba, B, 17, 0.03)
    a, b = _loop_solver(ba, B, x0, traj, pp), _loop_solver(ba, B, x0, traj, pp)
    for s in (a, b):
        s.set_delay(np.arange(B) % 4, comp=2)
    t, want = ba.BatchTrack(B), ba.BatchTrack(B)
    a.closed_loop_track(t, ticks, line0=line0, chunk=5)
    ul, xl, sl = b.closed_loop(ticks, line0=line0)
    assert a.get_x0().tobytes() == b.get_x0().tobytes() and a.results().tobytes() == b.results().tobytes()
    assert np.array_equal(a.delay_queue(), b.delay_queue()) and np.array_equal(a.delay_predicted(), b.delay_predicted())
    want.accumulate(xl[1:], ul, sl, traj, line0 + 1)                   # the true state after tick k against row line0 + k + 1, whatever comp is
    assert t.stats().tobytes() == want.stats().tobytes()
    assert (t.stats()["ticks"] == ticks).all()
    # the windows did start comp rows ahead: the loop through the public calls with the shifted window reproduces the log
    c = _loop_solver(ba, B, x0, traj, pp); c.set_delay(np.arange(B) % 4, comp=2)
    for k in range(ticks):
        c.set_yref_from_trajectory(line0 + k + 2, 16); c.solve(); c.plant_step(0.05, 1)
        assert np.array_equal(c.results()["u0"], ul[k]) and np.array_equal(c.get_x0(), xl[k + 1]), k
    for o in (a, b, c, t, want):
        o.close()
