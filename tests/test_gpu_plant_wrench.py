"""GPU tests of the plant under a time-varying world-frame wrench (brov_plant_wrench_*, plant_wrench_kernel) and of the DOB loop on the
device (brov_closed_loop_dob), against tests/wrench_restatement.py, the oracle's model / RTI step / EKF, and the call sequences the
loops replace."""
import math
import os

import numpy as np
import pytest

from oracle import trajectory_oracle as T
from oracle.oracle_ffi import EkfOracle
from wrench_restatement import WrenchRestatement, plant_step, cpu_dob_loop

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrench_tables.npz")
PERIODIC = dict(seed=0xC0FFEE123456789, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


def _modes(B, rng):
    """(name, device setter arguments, restatement) of the three modes, wrench magnitudes well below the 300 of the plant test"""
    tab = np.load(GOLDEN)["table"]
    wc = rng.uniform(-100, 100, (B, 6)); wc[:, 3:] *= 0.05
    gain = rng.uniform(-5, 5, B)
    return [("constant", dict(constant=wc), WrenchRestatement(B).constant(wc)),
            ("periodic", dict(periodic=PERIODIC), WrenchRestatement(B).periodic(**PERIODIC)),
            ("table", dict(table=tab, gain=gain), WrenchRestatement(B).table(tab, gain))]


def test_device_generator_matches_the_restatement(ba):
    B = 256
    rng = np.random.default_rng(1)
    s = ba.BatchSolver(B, ba.SolverOptions(10))
    assert s.plant_wrench_mode() == ba.WRENCH_OFF and not s.plant_wrench(3).any()
    for name, kw, r in _modes(B, rng):
        s.set_plant_wrench(**kw)
        worst = 0.0
        for k in list(range(201)) + ([495, 496, 100000] if name == "table" else []):
            wg, wr = s.plant_wrench(k), r.wrench(k)
            if name != "periodic":
                assert np.array_equal(wg, wr), (name, k)
                continue
            np.testing.assert_allclose(wg, wr, rtol=1e-14, atol=0, err_msg=f"tick {k}")
            assert not wg[:, 3:5].any() and np.array_equal(wg[:, 5], wg[:, 1] / 3.0)
            sn = r.sin_phase(k)
            if abs(sn) > 0.1:      # the amplitudes, with the restatement's own sin divided out
                A = r.amplitudes(k)
                np.testing.assert_allclose(wg[:, :3] / sn, A[:, :3], rtol=1e-14, atol=0, err_msg=f"tick {k}")
                worst = max(worst, np.abs(wg[:, :3] / sn / A[:, :3] - 1).max())
                assert (wg[:, :3] / sn).min() > 3.0 * (1 - 1e-14) and (wg[:, :3] / sn).max() < 6.0
        if name == "periodic":
            print(f"periodic: worst relative amplitude error {worst:.2e}")
    # the table without a gain, and evaluation moves nothing
    tab = np.load(GOLDEN)["table"]
    s.set_plant_wrench(table=tab)
    assert np.array_equal(s.plant_wrench(77), np.tile(tab[77], (B, 1))) and s.plant_wrench_tick() == 0
    # arguments
    with pytest.raises(RuntimeError):
        s.plant_wrench_seek(-1)
    with pytest.raises(RuntimeError):
        s.set_plant_wrench(periodic=dict(tz_div=0.0))
    s.set_plant_wrench(periodic=dict(dphi=1.0))
    with pytest.raises(RuntimeError):
        s.plant_wrench_seek(int(2 ** 22 * math.pi) + 8)        # half-period index beyond its 22 bits
    s.close()


@pytest.mark.parametrize("substeps", [1, 4])
def test_plant_step_under_a_wrench_matches_the_restated_rk4(ba, oracle, substeps):
    N, B = 20, 96
    rng = np.random.default_rng(5)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * 0.1
    x0[:, 3:5] += rng.uniform(-0.4, 0.4, (B, 2))          # roll and pitch of a few tenths of a radian: the projection matters
    p = np.tile(ba.P_NOMINAL, (B, 1)); p[:, :4] = rng.uniform(-100, 100, (B, 4))
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(p); s.set_yref(traj[:N + 1])
    s.solve()
    u0 = s.results()["u0"]
    for name, kw, r in _modes(B, rng):
        s.set_plant_wrench(**kw)
        for tick in (13, 140):
            s.set_x0(x0); s.plant_wrench_seek(tick)
            s.plant_step(0.05, substeps)
            x1 = s.get_x0()
            assert s.plant_wrench_tick() == tick + 1
            w = r.wrench(tick)
            assert np.abs(w).max() > 1.0 and np.abs(w).max() < 300.0
            err = np.abs(x1 - plant_step(oracle, x0, u0, p, w, 0.05, substeps)).max()
            print(f"{name} tick {tick} substeps {substeps}: |x_gpu - x_restated|_inf = {err:.2e}")
            assert err < 1e-12, (name, tick, err)
            # ... and the wrench is felt: the step without it lands elsewhere
            assert np.abs(x1 - plant_step(oracle, x0, u0, p, np.zeros((B, 6)), 0.05, substeps)).max() > 1e-6
    s.close()


def _loop_solver(ba, B, N, x0, traj, pp):
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(pp); s.set_trajectory(traj)
    return s


def test_mode_off_is_the_parent_path_and_a_zero_wrench_agrees_with_it(ba):
    N, B, ticks = 20, 48, 8
    rng = np.random.default_rng(8)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = rng.uniform(-100, 100, (B, 4))
    parent = _loop_solver(ba, B, N, x0, traj, pp)          # never touches the wrench API
    off = _loop_solver(ba, B, N, x0, traj, pp)
    off.set_plant_wrench(constant=rng.uniform(-50, 50, (B, 6))); off.set_plant_wrench(periodic=PERIODIC); off.plant_wrench_off()
    zero = _loop_solver(ba, B, N, x0, traj, pp)
    zero.set_plant_wrench(constant=np.zeros(6))
    assert off.plant_wrench_mode() == ba.WRENCH_OFF and zero.plant_wrench_mode() == ba.WRENCH_CONSTANT
    # one plant step behind one solve
    for s in (parent, off, zero):
        s.set_yref(traj[:N + 1]); s.solve(); s.plant_step(0.05, 2)
    xp, xo, xz = parent.get_x0(), off.get_x0(), zero.get_x0()
    assert np.array_equal(xp, xo)
    assert np.abs(xz - xp).max() < 1e-12
    # the closed loop
    for s in (parent, off, zero):
        s.set_x0(x0); s.init_iterate_default()
    lp = parent.closed_loop(ticks, line0=3)
    lo = off.closed_loop(ticks, line0=3, log_wrench=True)
    lz = zero.closed_loop(ticks, line0=3, log_wrench=True)
    assert parent.last_kernel_path() == off.last_kernel_path() == zero.last_kernel_path() == ba.PATH_FUSED
    for a, b in zip(lp, lo[:3]):
        assert np.array_equal(a, b)
    assert not lo[3].any() and not lz[3].any()
    assert np.array_equal(parent.get_x0(), off.get_x0()) and np.array_equal(parent.results(), off.results())
    assert np.array_equal(lp[2], lz[2])
    print(f"zero wrench against the parent path: |du| = {np.abs(lp[0] - lz[0]).max():.2e}, |dx| = {np.abs(lp[1] - lz[1]).max():.2e}")
    assert np.abs(lp[0] - lz[0]).max() < 1e-12 and np.abs(lp[1] - lz[1]).max() < 1e-12
    assert off.plant_wrench_tick() == zero.plant_wrench_tick() == ticks + 1
    for s in (parent, off, zero):
        s.close()


def test_closed_loop_under_the_periodic_wrench_equals_the_call_sequence(ba):
    N, B, ticks, line0 = 20, 40, 10, 2
    rng = np.random.default_rng(9)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = rng.uniform(-30, 30, (B, 4))
    a = _loop_solver(ba, B, N, x0, traj, pp); a.set_plant_wrench(periodic=PERIODIC); a.plant_wrench_seek(20)
    b = _loop_solver(ba, B, N, x0, traj, pp); b.set_plant_wrench(periodic=PERIODIC); b.plant_wrench_seek(20)
    ul, xl, sl, wl = a.closed_loop(ticks, line0=line0, substeps=2, log_wrench=True)
    assert a.plant_wrench_tick() == 20 + ticks and a.last_kernel_path() == ba.PATH_FUSED
    assert np.array_equal(xl[0], x0) and np.abs(wl).max() > 1.0
    for k in range(ticks):
        b.set_yref_from_trajectory(line0 + k, 16); b.solve()
        r = b.results()
        w = b.plant_wrench(b.plant_wrench_tick())
        b.plant_step(0.05, 2)
        assert np.array_equal(r["u0"], ul[k]) and np.array_equal(r["status"], sl[k]) and np.array_equal(w, wl[k]), k
        assert np.array_equal(b.get_x0(), xl[k + 1]), k
    assert b.plant_wrench_tick() == 20 + ticks
    assert np.all(sl == 0)
    # from the same start and the same tick the run repeats bit for bit: the generator keeps no state
    a.set_x0(x0); a.init_iterate_default(); a.plant_wrench_seek(20)
    again = a.closed_loop(ticks, line0=line0, substeps=2, log_wrench=True)
    for p, q in zip((ul, xl, sl, wl), again):
        assert np.array_equal(p, q)
    # and from another tick it does not
    a.set_x0(x0); a.init_iterate_default(); a.plant_wrench_seek(21)
    assert not np.array_equal(a.closed_loop(ticks, line0=line0, substeps=2, log_wrench=True)[1], xl)
    a.close(); b.close()


def _ekf_pair(ba, B):
    """device observer and oracle EKF for the device plant: the OCP model itself, unit scaling, no roll / pitch thrust (see
    brov_ekf_apply_to_solver in include/bluerov2_nmpc.h and tests/test_gpu_ekf.py::test_device_loop_with_solver)"""
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    orc = EkfOracle(); orc.par.compensate_coef = 1.0; orc.par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
        orc.par.K[j] = 0.0
    return (ba.BatchEkf(B, par) if B else None), orc


@pytest.mark.parametrize("with_rls", [False, True])
def test_closed_loop_dob_equals_the_five_call_sequence(ba, with_rls):
    N, B, ticks, line0 = 20, 24, 12, 1
    rng = np.random.default_rng(12)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :6] += rng.normal(size=(B, 6)) * 0.03
    pp = np.tile(ba.P_NOMINAL, (B, 1))
    out = []
    for fused in (True, False):
        s = _loop_solver(ba, B, N, x0, traj, pp); s.set_plant_wrench(periodic=PERIODIC)
        e, _ = _ekf_pair(ba, B)
        r = None
        if with_rls:
            rp = ba.RlsParams.default(); rp.compensate_coef = 1.0; rp.rotor_constant = 1.0
            r = ba.BatchRls(B, rp)
        if fused:
            log = s.closed_loop_dob(e, r, ba.APPLY_DISTURBANCE, ticks=ticks, line0=line0, substeps=1)
        else:
            log = dict(u=[], x=[s.get_x0()], status=[], wrench=[], est=[])
            for k in range(ticks):
                s.set_yref_from_trajectory(line0 + k, 16); s.solve()
                log["wrench"].append(s.plant_wrench(s.plant_wrench_tick()))
                s.plant_step(0.05, 1)
                e.update_from_solver(s)
                if r is None:
                    e.apply_to_solver(s)
                else:
                    r.update_from_ekf(e, s); r.apply_to_solver(s, ba.APPLY_DISTURBANCE)
                res = s.results()
                log["u"].append(res["u0"].copy()); log["status"].append(res["status"].copy()); log["x"].append(s.get_x0())
                log["est"].append(e.state()[0][:, 12:].copy())
            log = {k: np.array(v) for k, v in log.items()}
        out.append((log, s.get_params(), s.get_x0(), e.state(), s.plant_wrench_tick()))
        s.close(); e.close()
        if r is not None:
            r.close()
    (la, pa, xa, ea, ta), (lb, pb, xb, eb, tb) = out
    for key in ("u", "x", "status", "wrench", "est"):
        assert np.array_equal(la[key], lb[key]), key
    assert np.array_equal(pa, pb) and np.array_equal(xa, xb) and np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1])
    assert ta == tb == ticks and np.all(la["status"] == 0) and np.abs(la["wrench"]).max() > 1.0
    assert np.abs(pa[:, :, :4]).max() > 0.1                   # the hand-off reached the controller's parameters


def test_closed_loop_dob_agrees_with_the_cpu_loop(ba, oracle):
    """The device DOB loop under the periodic wrench against the loop rebuilt on the CPU (oracle RTI step, restated plant, oracle EKF,
    hand-off), with the tolerances of tests/test_gpu_ekf.py::test_device_loop_with_solver: 1e-6 on the plant states, 1e-4 (+ 1e-5
    relative) on the disturbance estimate, 5e-3 (+ 1e-5 relative) on the parameters handed to the controller.  Unlike that test the
    two loops here never exchange a number: each closes through its own solver, plant and observer for all 30 ticks."""
    N, B, ticks = 20, 6, 30
    rng = np.random.default_rng(7)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :2] += rng.uniform(-0.3, 0.3, (B, 2))
    pp = np.tile(ba.P_NOMINAL, (B, 1))
    s = _loop_solver(ba, B, N, x0, traj, pp); s.set_plant_wrench(periodic=PERIODIC)
    e, eo = _ekf_pair(ba, B)
    log = s.closed_loop_dob(e, ticks=ticks)
    cpu = cpu_dob_loop(oracle, eo, WrenchRestatement(B).periodic(**PERIODIC), traj, x0, ba.P_NOMINAL, pp, N, ticks)
    assert np.all(log["status"] == 0) and np.all(cpu["status"] == 0)
    mp_gpu = s.get_params()[:, 0, :4]
    gx, ge, gp = np.abs(log["x"] - cpu["x"]).max(), np.abs(log["est"] - cpu["est"]).max(), np.abs(mp_gpu - cpu["mpc_p"][-1]).max()
    print(f"GPU loop against CPU loop over {ticks} ticks: |dx| = {gx:.2e}, |d est| = {ge:.2e}, |d mpc_p| = {gp:.2e}")
    np.testing.assert_allclose(log["wrench"], cpu["wrench"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(log["x"], cpu["x"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(log["est"], cpu["est"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(mp_gpu, cpu["mpc_p"][-1], rtol=1e-5, atol=5e-3)
    s.close(); e.close()


def test_compensation_helps_under_the_reference_constant_world_wrench(ba):
    """The reference's mode 1, (10, 10, 10, 0, 0, 0) N in the world frame, on the circle: the DOB loop (hand-off of the estimate to the
    controller) tracks better than the same loop without the hand-off.  Batch 4, 80 ticks, chosen on the CPU loop before any GPU run
    (DESIGN.md, section on the plant wrench): RMS position error 0.0913 m with the hand-off against 0.0996 m without, over a floor of
    0.087 m without any wrench.  Only the ordering is asserted here, and that every step succeeds."""
    N, B, ticks = 20, 4, 80
    rng = np.random.default_rng(21)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
    pp = np.tile(ba.P_NOMINAL, (B, 1))
    rms = {}
    for handoff in (True, False):
        s = _loop_solver(ba, B, N, x0, traj, pp); s.set_plant_wrench(constant=[10, 10, 10, 0, 0, 0])
        e, _ = _ekf_pair(ba, B)
        if handoff:
            log = s.closed_loop_dob(e, ticks=ticks)
            x, st = log["x"], log["status"]
        else:
            _, x, st, _ = s.closed_loop(ticks, log_wrench=True)
        assert np.all(st == 0)
        err = x[1:, :, :3] - traj[1:ticks + 1, None, :3]
        rms[handoff] = float(np.sqrt((err ** 2).sum(-1).mean()))
        s.close(); e.close()
    print(f"RMS position error under (10, 10, 10) N: {rms[True]:.4f} m compensated, {rms[False]:.4f} m uncompensated")
    assert rms[True] < rms[False]
