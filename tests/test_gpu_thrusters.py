"""GPU tests of the plant's thruster stage (brov_thruster_*, thruster_eval_kernel, plant_thruster_kernel) against tests/thruster_restatement.py,
the oracle's model / RTI step / EKF, and the call sequences the loops replace."""
import json
import os

import numpy as np
import pytest

from oracle import trajectory_oracle as T
from oracle.oracle_ffi import EkfOracle
from wrench_restatement import WrenchRestatement
from wrench_restatement import plant_step as plant_step_commanded
import thruster_restatement as TR
from thruster_restatement import ThrusterRestatement

pytestmark = pytest.mark.gpu
TAM = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thruster_tam.json")))
PERIODIC = dict(seed=0xC0FFEE123456789, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


def _same(a, b):
    """equal values, NaNs compared by position, zeros by sign"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan], b[~nan]) and \
        np.array_equal(np.signbit(a[~nan]), np.signbit(b[~nan]))


def _same_stats(st, r):
    return np.array_equal(st["clip_ticks"], r.clip_ticks) and np.array_equal(st["lost_sq"], r.lost_sq) and st["steps"] == r.steps


def _loop_solver(ba, B, N, x0, traj, pp):
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(pp); s.set_trajectory(traj)
    return s


def _ekf_pair(ba, B):
    """device observer and oracle EKF for the device plant, as tests/test_gpu_plant_wrench.py::_ekf_pair configures them"""
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    orc = EkfOracle(); orc.par.compensate_coef = 1.0; orc.par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
        orc.par.K[j] = 0.0
    return (ba.BatchEkf(B, par) if B else None), orc


# ---- 1. the stage, bit for bit ------------------------------------------------------------------------------------------------------------
def test_stage_matches_the_restatement_bit_for_bit(ba):
    B = 130                                                          # one full block plus two lanes
    rng = np.random.default_rng(3)
    lo, hi = rng.uniform(-3000, -500, 6), rng.uniform(500, 3000, 6)
    cmd = rng.uniform(-6000, 6000, (B, 6))
    cmd[0, 0] = np.nan; cmd[129, 5] = np.nan; cmd[1, 1] = 0.0; cmd[2, 2] = -0.0; cmd[3] = lo; cmd[4] = hi; cmd[128] = hi; cmd[129, :3] = lo[:3]
    K = rng.normal(size=(6, 6))
    gain, bias = rng.uniform(-1, 2, (B, 6)), rng.uniform(-50, 50, (B, 6))
    onset = rng.choice(np.array([0, 7, 2 ** 40], dtype=np.int64), B)
    s = ba.BatchSolver(B, ba.SolverOptions(10))
    assert not s.thrusters_enabled()
    s.set_thrusters(K=K, lo=lo, hi=hi, gain=gain, bias=bias, onset=onset)
    assert s.thrusters_enabled()
    r = ThrusterRestatement(B, K, lo, hi, gain, bias, onset)
    seen = set()
    for tick in (0, 6, 7, 2 ** 40):
        a, g = s.thruster_eval(tick, cmd)
        ar, gr = r.stage(tick, cmd)
        assert _same(a, ar), tick
        assert _same(g, gr), tick
        seen.add(a[~np.isnan(a)].tobytes())
    assert len(seen) == 3                                            # ticks 0 and 6 agree; 7 and 2^40 each bring an onset group in
    assert np.isnan(a[0, 0]) and np.isnan(a[129, 5]) and np.isnan(g[0]).all() and not np.isnan(a[1:129]).any()
    # evaluation advances no counter and touches no statistic
    st = s.thruster_stats()
    assert s.plant_wrench_tick() == 0 and st["steps"] == 0 and not st["clip_ticks"].any() and not st["lost_sq"].any()
    assert not s.thruster_last().any()
    s.close()


# ---- 2. the plant step against the restated RK4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 4])
def test_plant_step_behind_the_stage_matches_the_restated_rk4(ba, oracle, substeps):
    N, B, tick = 20, 96, 13
    rng = np.random.default_rng(5)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * 0.1
    x0[:, 3:5] += rng.uniform(-0.4, 0.4, (B, 2))
    p = np.tile(ba.P_NOMINAL, (B, 1)); p[:, :4] = rng.uniform(-100, 100, (B, 4))
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(p); s.set_yref(traj[:N + 1])
    s.solve()
    u0, t = s.results()["u0"], s.thrusts()
    lim = float(np.median(np.abs(t)))                                # about half of the 6 B commands clip, by construction
    clipped = np.mean(np.abs(t) > lim)
    print(f"limits +-{lim:.1f}: {100 * clipped:.1f} % of the commands clip")
    assert 0.25 < clipped < 0.75
    gain = rng.uniform(0, 1, (B, 6))
    onset = np.where(np.arange(B) % 2 == 0, 5, 100)                   # half the instances are past their onset at the tick
    K_tam = TR.K_MODEL.copy(); K_tam[3:5] = np.array(TAM["tam"])[3:5]
    wr = WrenchRestatement(B).periodic(**PERIODIC)
    x_plain = plant_step_commanded(oracle, x0, u0, p, np.zeros((B, 6)), 0.05, substeps)
    for name, K, wrench in (("model K", None, False), ("TAM roll / pitch rows", K_tam, False), ("model K + periodic wrench", None, True)):
        if wrench:
            s.set_plant_wrench(periodic=PERIODIC)
        else:
            s.plant_wrench_off()
        s.set_thrusters(K=K, lo=-lim, hi=lim, gain=gain, onset=onset)
        s.set_x0(x0); s.plant_wrench_seek(tick)
        s.plant_step(0.05, substeps)
        x1 = s.get_x0()
        assert s.plant_wrench_tick() == tick + 1
        r = ThrusterRestatement(B, K, -lim, lim, gain, None, onset)
        a, g = r.step(tick, t)
        w = wr.wrench(tick) if wrench else None
        err = np.abs(x1 - TR.plant_step(oracle, x0, p, g, w, 0.05, substeps)).max()
        print(f"{name}, substeps {substeps}: |x_gpu - x_restated|_inf = {err:.2e}")
        assert err < 1e-12, (name, err)
        assert np.array_equal(s.thruster_last(), a), name
        assert _same_stats(s.thruster_stats(), r), name
        assert r.clip_ticks.sum() == int(round(clipped * 6 * B)) and r.lost_sq[::2].min() > 0.0   # (even instances: past their onset)
        if name != "model K":
            assert np.abs(g[:, 3:5]).max() > 1.0 or wrench               # the roll / pitch rows are felt
        # ... and the stage is felt: the step with the commanded wrench lands elsewhere
        assert np.abs(x1 - x_plain).max() > 1e-6
    s.close()


def test_roll_pitch_disturbance_moments_add_to_the_stage_moments(ba, oracle):
    """6-disturbance variant: the plant's roll / pitch moments are ADDED to the moments the TAM's rows 3 and 4 give the thrusters.  The same
    comparison as above (the restated RK4 with drp = (g3, g4) + the moments), held to the same 1e-12."""
    N, B, tick, substeps = 20, 40, 2, 2
    rng = np.random.default_rng(17)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * 0.1
    p = np.tile(ba.P_NOMINAL, (B, 1)); p[:, :4] = rng.uniform(-100, 100, (B, 4))
    rp = rng.uniform(-5, 5, (B, 2))
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.enable_dist6(); s.set_yref(traj[:N + 1])
    s.solve()
    s.set_plant_params(p); s.set_plant_rp_disturbance(rp)
    t = s.thrusts()
    lim = float(np.median(np.abs(t)))
    gain = rng.uniform(0, 1, (B, 6))
    K_tam = TR.K_MODEL.copy(); K_tam[3:5] = np.array(TAM["tam"])[3:5]
    s.set_thrusters(K=K_tam, lo=-lim, hi=lim, gain=gain)
    s.plant_wrench_seek(tick); s.plant_step(0.05, substeps)
    x1 = s.get_x0()
    a, g = ThrusterRestatement(B, K_tam, -lim, lim, gain).step(tick, t)
    err = np.abs(x1 - TR.plant_step(oracle, x0, p, g, None, 0.05, substeps, prp=rp)).max()
    print(f"TAM rows + roll / pitch disturbance moments: |x_gpu - x_restated|_inf = {err:.2e}")
    assert err < 1e-12 and np.abs(g[:, 3:5]).max() > 1.0
    assert np.abs(x1 - TR.plant_step(oracle, x0, p, g, None, 0.05, substeps)).max() > 1e-6      # without the moments: elsewhere
    assert np.array_equal(s.thruster_last(), a)
    s.close()


# ---- 3. off is the parent path; healthy is the parent path to rounding ----------------------------------------------------------------------
def test_off_is_the_parent_path_and_healthy_thrusters_agree_with_it(ba):
    N, B, ticks = 20, 48, 8
    rng = np.random.default_rng(8)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = rng.uniform(-100, 100, (B, 4))
    parent = _loop_solver(ba, B, N, x0, traj, pp)                    # never touches the thruster API
    off = _loop_solver(ba, B, N, x0, traj, pp)
    off.set_thrusters(lo=-10.0, hi=10.0, gain=rng.uniform(0, 1, (B, 6)), bias=3.0); off.thrusters_off()
    healthy = _loop_solver(ba, B, N, x0, traj, pp)
    healthy.set_thrusters()                                          # the model's K, no limits, gain 1, bias 0
    assert not parent.thrusters_enabled() and not off.thrusters_enabled() and healthy.thrusters_enabled()
    for s in (parent, off, healthy):
        s.set_yref(traj[:N + 1]); s.solve(); s.plant_step(0.05, 2)
    xp, xo, xh = parent.get_x0(), off.get_x0(), healthy.get_x0()
    assert np.array_equal(xp, xo)
    print(f"healthy thrusters against the parent path, one step: |dx| = {np.abs(xh - xp).max():.2e}")
    assert np.abs(xh - xp).max() < 1e-12
    assert np.array_equal(healthy.thruster_last(), healthy.thrusts())
    for s in (parent, off, healthy):
        s.set_x0(x0); s.init_iterate_default()
    lp = parent.closed_loop(ticks, line0=3)
    lo = off.closed_loop(ticks, line0=3)
    assert parent.last_kernel_path() == off.last_kernel_path() == ba.PATH_FUSED     # the one-launch loop
    lh = healthy.closed_loop(ticks, line0=3)
    for a, b in zip(lp, lo):
        assert np.array_equal(a, b)
    assert np.array_equal(parent.get_x0(), off.get_x0()) and np.array_equal(parent.results(), off.results())
    assert np.array_equal(lp[2], lh[2])
    print(f"healthy thrusters against the parent path, {ticks} ticks: |du| = {np.abs(lp[0] - lh[0]).max():.2e}, |dx| = {np.abs(lp[1] - lh[1]).max():.2e}")
    assert np.abs(lp[0] - lh[0]).max() < 1e-12 and np.abs(lp[1] - lh[1]).max() < 1e-12
    st = healthy.thruster_stats()
    assert st["steps"] == ticks + 1 and not st["clip_ticks"].any() and np.all(st["lost_sq"] == 0.0)
    assert off.thruster_stats()["steps"] == 0                          # off: readable, and nothing was counted
    assert parent.plant_wrench_tick() == off.plant_wrench_tick() == healthy.plant_wrench_tick() == ticks + 1
    for s in (parent, off, healthy):
        s.close()


# ---- 4. the loops equal their call sequences, bit for bit -----------------------------------------------------------------------------------
def _faulty(s, B):
    gain = np.ones((B, 6)); gain[::2, 0] = 0.0                         # thruster 0 dead ...
    onset = np.where(np.arange(B) % 2 == 0, 4, 0)                       # ... from tick 4 on, in half the instances
    s.set_thrusters(lo=-100.0, hi=100.0, gain=gain, onset=onset)
    return ThrusterRestatement(B, None, -100.0, 100.0, gain, None, onset)


@pytest.mark.parametrize("kind", ["plain", "dob", "dob_rls"])
def test_loops_behind_the_stage_equal_their_call_sequences(ba, kind):
    N, B, ticks, line0 = 20, 24, 12, 1
    rng = np.random.default_rng(12)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :6] += rng.normal(size=(B, 6)) * 0.03
    pp = np.tile(ba.P_NOMINAL, (B, 1))

    def observer():
        if kind == "plain":
            return None, None
        e, _ = _ekf_pair(ba, B)
        r = None
        if kind == "dob_rls":
            rp = ba.RlsParams.default(); rp.compensate_coef = 1.0; rp.rotor_constant = 1.0
            r = ba.BatchRls(B, rp)
        return e, r

    def loop(s, e, r):
        if kind == "plain":
            ul, xl, sl, wl = s.closed_loop(ticks, line0=line0, log_wrench=True)
            return dict(u=ul, x=xl, status=sl, wrench=wl)
        return s.closed_loop_dob(e, r, ba.APPLY_DISTURBANCE, ticks=ticks, line0=line0)

    out = []
    for fused in (True, False):
        s = _loop_solver(ba, B, N, x0, traj, pp); s.set_plant_wrench(periodic=PERIODIC)
        rt = _faulty(s, B)
        e, r = observer()
        if fused:
            log = loop(s, e, r)
        else:
            log = dict(u=[], x=[s.get_x0()], status=[], wrench=[], est=[])
            for k in range(ticks):
                s.set_yref_from_trajectory(line0 + k, 16); s.solve()
                tick = s.plant_wrench_tick()
                log["wrench"].append(s.plant_wrench(tick))
                s.plant_step(0.05, 1)
                a, _ = rt.step(tick, s.thrusts())
                assert np.array_equal(s.thruster_last(), a), k             # the applied thrusts of THIS tick
                if e is not None:
                    e.update_from_solver(s)
                    if r is None:
                        e.apply_to_solver(s)
                    else:
                        r.update_from_ekf(e, s); r.apply_to_solver(s, ba.APPLY_DISTURBANCE)
                    log["est"].append(e.state()[0][:, 12:].copy())
                res = s.results()
                log["u"].append(res["u0"].copy()); log["status"].append(res["status"].copy()); log["x"].append(s.get_x0())
            log = {k: np.array(v) for k, v in log.items() if len(v)}
            assert _same_stats(s.thruster_stats(), rt)                   # the device statistics are the restatement's
            assert rt.clip_ticks.sum() > 0 and rt.lost_sq[::2].min() > 0.0   # (even instances: thruster 0 dead from tick 4)
        out.append((log, s.get_params(), s.get_x0(), e.state() if e is not None else (), s.thruster_stats(), s.plant_wrench_tick()))
        if fused and kind == "plain":
            # from the same start and tick the run reproduces bit for bit: the stage keeps no state
            s.set_x0(x0); s.init_iterate_default(); s.plant_wrench_seek(0); s.thruster_reset_stats()
            again = loop(s, e, r)
            for key in log:
                assert np.array_equal(log[key], again[key]), key
            assert np.array_equal(s.thruster_stats()["lost_sq"], out[0][4]["lost_sq"])
            # the scored loop in chunks of 5 against the unchunked one
            recs = []
            for chunk in (5, 0):
                s.set_x0(x0); s.init_iterate_default(); s.plant_wrench_seek(0); s.thruster_reset_stats()
                t = ba.BatchTrack(B)
                s.closed_loop_track(t, ticks, line0=line0, chunk=chunk)
                recs.append((t.stats().tobytes(), s.thruster_stats(), s.get_x0()))
                t.close()
            assert recs[0][0] == recs[1][0] and np.array_equal(recs[0][2], recs[1][2]) and np.array_equal(recs[0][2], out[0][2])
            for st in (recs[0][1], recs[1][1]):
                assert np.array_equal(st["clip_ticks"], out[0][4]["clip_ticks"]) and np.array_equal(st["lost_sq"], out[0][4]["lost_sq"])
                assert st["steps"] == ticks
        for o in (s, e, r):
            if o is not None:
                o.close()
    (la, pa, xa, ea, sa, ta), (lb, pb, xb, eb, sb, tb) = out
    assert set(la) == set(lb)
    for key in la:
        assert np.array_equal(la[key], lb[key]), key
    assert np.array_equal(pa, pb) and np.array_equal(xa, xb)
    for p, q in zip(ea, eb):
        assert np.array_equal(p, q)
    assert np.array_equal(sa["clip_ticks"], sb["clip_ticks"]) and np.array_equal(sa["lost_sq"], sb["lost_sq"]) and sa["steps"] == sb["steps"] == ticks
    assert ta == tb == ticks and np.all(la["status"] == 0) and np.abs(la["wrench"]).max() > 1.0


# ---- 5. the device loop against the CPU loop ------------------------------------------------------------------------------------------------
def _start(ba, B):
    rng = np.random.default_rng(21)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
    return traj, x0, np.tile(ba.P_NOMINAL, (B, 1))


def test_dob_loop_behind_the_stage_agrees_with_the_cpu_loop(ba, oracle):
    """The device DOB loop with limits of +-100 against the loop rebuilt on the CPU (oracle RTI step, restated stage and plant, oracle EKF
    fed with the commanded thrusts, hand-off), with the tolerances of tests/test_gpu_plant_wrench.py::test_closed_loop_dob_agrees_with_the_cpu_loop."""
    N, B, ticks = 20, 4, 30
    traj, x0, pp = _start(ba, B)
    _, eo = _ekf_pair(ba, 0)
    rt = ThrusterRestatement(B, None, -100.0, 100.0)
    cpu = TR.cpu_thruster_loop(oracle, eo, rt, traj, x0, ba.P_NOMINAL, pp, N, ticks)
    frac = rt.clip_ticks.sum() / (6.0 * B * ticks)
    print(f"CPU loop: {rt.clip_ticks.sum()} of {6 * B * ticks} commands clip")
    assert 0.01 < frac < 0.5
    s = _loop_solver(ba, B, N, x0, traj, pp); s.set_thrusters(lo=-100.0, hi=100.0)
    e, _ = _ekf_pair(ba, B)
    log = s.closed_loop_dob(e, ticks=ticks)
    assert np.all(log["status"] == 0) and np.all(cpu["status"] == 0)
    mp_gpu = s.get_params()[:, 0, :4]
    gx, ge, gp = np.abs(log["x"] - cpu["x"]).max(), np.abs(log["est"] - cpu["est"]).max(), np.abs(mp_gpu - cpu["mpc_p"][-1]).max()
    print(f"GPU loop against CPU loop over {ticks} ticks: |dx| = {gx:.2e}, |d est| = {ge:.2e}, |d mpc_p| = {gp:.2e}; "
          f"clipped on the device: {s.thruster_stats()['clip_ticks'].sum()}")
    np.testing.assert_allclose(log["x"], cpu["x"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(log["est"], cpu["est"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(mp_gpu, cpu["mpc_p"][-1], rtol=1e-5, atol=5e-3)
    s.close(); e.close()


# ---- 6. the point of it -----------------------------------------------------------------------------------------------------------------------
def test_the_observer_compensates_a_dead_thruster(ba):
    """Thruster 0 dead from tick 10, no limits, on the circle: the DOB loop (the estimate handed to the controller) tracks better than the
    same loop without the hand-off.  Batch 4, 80 ticks, chosen on the CPU loop before any GPU run: RMS position
    error 0.0874 m with the hand-off against 0.1495 m without, over a healthy floor of 0.0871 m.  Only the ordering is asserted, and that
    every step succeeds.  (A thruster at half gain is NOT asserted: there the uncompensated controller is the better one on the CPU loop.)"""
    N, B, ticks = 20, 4, 80
    traj, x0, pp = _start(ba, B)
    gain = np.ones(6); gain[0] = 0.0
    rms = {}
    for handoff in (True, False):
        s = _loop_solver(ba, B, N, x0, traj, pp); s.set_thrusters(gain=gain, onset=10)
        e, _ = _ekf_pair(ba, B)
        if handoff:
            log = s.closed_loop_dob(e, ticks=ticks)
            x, st = log["x"], log["status"]
        else:
            _, x, st = s.closed_loop(ticks)
        assert np.all(st == 0)
        assert s.thruster_stats()["steps"] == ticks and s.thruster_stats()["lost_sq"].min() > 0.0
        err = x[1:, :, :3] - traj[1:ticks + 1, None, :3]
        rms[handoff] = float(np.sqrt((err ** 2).sum(-1).mean()))
        s.close(); e.close()
    print(f"RMS position error with thruster 0 dead from tick 10: {rms[True]:.4f} m with the hand-off, {rms[False]:.4f} m without")
    assert rms[True] < rms[False]


# ---- 7. arguments and the fleet ---------------------------------------------------------------------------------------------------------------
def test_refused_arguments_change_nothing_and_the_fleet_refuses_the_stage(ba):
    B, N = 4, 10
    rng = np.random.default_rng(2)
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
    s.set_params(ba.P_NOMINAL)
    gain = rng.uniform(0, 1, (B, 6))
    s.set_thrusters(lo=-50.0, hi=80.0, gain=gain, bias=1.0, onset=3)
    cmd = rng.uniform(-200, 200, (B, 6))
    before = s.thruster_eval(5, cmd)
    bad_gain = gain.copy(); bad_gain[1, 2] = np.nan
    hi_nan = np.full(6, 80.0); hi_nan[4] = np.nan
    for kw, text in ((dict(lo=10.0, hi=-10.0), r"brov_thruster_set_host: lo\[i\] > hi\[i\]"), (dict(gain=bad_gain), "brov_thruster_set_host: K, gain and bias must be finite"),
                     (dict(bias=np.inf), "brov_thruster_set_host: K, gain and bias must be finite"), (dict(K=np.full((6, 6), np.inf)), "must be finite"),
                     (dict(hi=hi_nan), "brov_thruster_set_host: a thrust limit is NaN"), (dict(onset=[0, 1, -1, 2]), "brov_thruster_set_host: negative onset")):
        with pytest.raises(RuntimeError, match=text):
            s.set_thrusters(**kw)
    with pytest.raises(RuntimeError, match="brov_thruster_eval_host: negative tick"):
        s.thruster_eval(-1, cmd)
    with pytest.raises(RuntimeError, match="brov_thruster_last_seconds: no plant step"):
        s.thruster_last_seconds()
    after = s.thruster_eval(5, cmd)
    assert s.thrusters_enabled() and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    r = ThrusterRestatement(B, None, -50.0, 80.0, gain, 1.0, 3)
    assert np.array_equal(after[0], r.stage(5, cmd)[0]) and np.array_equal(after[1], r.stage(5, cmd)[1])
    # the fleet has its own plant kernel, which knows no thrusters
    x0 = np.zeros((B, 12)); x0[:, 2] = -20.0
    s.set_x0(x0); s.set_candidate_params("circle", np.full(B, 2.0), np.full(B, 0.5), np.zeros(B))
    f = ba.Fleet(s, 2)
    for call in (lambda: f.step(), lambda: f.closed_loop(2, dt_ref=0.05, dt_node=0.05), lambda: f.closed_loop_dob(None, 2, dt_ref=0.05, dt_node=0.05)):
        with pytest.raises(RuntimeError, match="thruster stage"):
            call()
    s.thrusters_off()
    u, x, st, win = f.closed_loop(2, dt_ref=0.05, dt_node=0.05)
    assert np.isfinite(x).all()
    f.step()
    s.plant_step(0.05, 1)                                              # the solver's own plant, stage off: nothing is counted or timed
    assert s.thruster_stats()["steps"] == 0
    s.set_thrusters(); s.plant_step(0.05, 1)
    assert s.thruster_stats()["steps"] == 1 and 0.0 < s.thruster_last_seconds() < 1.0
    f.close(); s.close()
