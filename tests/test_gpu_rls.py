"""Batched RLS-FF parameter estimator (brov_rls_*, reference BLUEROV2_AMPC::RLSFF, bluerov2_ampc.cpp:731-1046) on the GPU against the
CPU restatement (tests/rlsff_restatement.py): theta, P, lambda, F and e bit for bit, wf_env to 1e-13 (sin / cos), the hand-off to
the solver, and the on-device AMPC tick solve -> plant -> EKF -> RLS -> parameters."""
import numpy as np
import pytest

from rlsff_restatement import RlsffRestatement, LAM_DOWN, LAM_FLOOR, LAM_UP, LAM_CEIL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    import bluerov2_amd
    return bluerov2_amd


def scenario(B, ticks, seed):
    """per-tick inputs (y, acc, vel, rpy): per-instance theta*, smooth regressors plus noise, a theta* step at tick 150, and a
    growing target on the yaw axis of every eighth instance (instance 0 included) from tick 200 on"""
    rng = np.random.default_rng(seed)
    ts = [rng.normal(size=(B, 4, 4)) * 3, rng.normal(size=(B, 4, 4)) * 3]
    ph = rng.uniform(0, 2 * np.pi, (B, 4, 3))
    w = rng.uniform(0.5, 4.0, (B, 4, 3))
    grow = np.zeros(B, dtype=bool); grow[::8] = True
    for k in range(ticks):
        t = 0.05 * k
        acc = np.sin(w[..., 0] * t + ph[..., 0]) + 0.3 * rng.normal(size=(B, 4)) * 0.1
        vel = 0.8 * np.cos(w[..., 1] * t + ph[..., 1]) + 0.2 * np.sin(w[..., 2] * t + ph[..., 2]) + rng.normal(size=(B, 4)) * 0.01
        th = ts[0] if k < 150 else ts[1]
        x = [acc, vel, np.ones_like(vel), vel * np.abs(vel)]
        y = x[0] * th[:, :, 0] + x[1] * th[:, :, 1] + x[2] * th[:, :, 2] + x[3] * th[:, :, 3] + rng.normal(size=(B, 4)) * 0.05
        if k >= 200:
            y[grow, 3] = 2.0 ** (k - 200)
        rpy = rng.uniform(-0.4, 0.4, (B, 3))
        yield k, y, acc, vel, rpy


def assert_matches(r, ref, what):
    th, P, lam, F, e = r.state()
    for name, a, b in (("theta", th, ref.theta), ("P", P, ref.P), ("lambda", lam, ref.lam), ("F", F, ref.F), ("e", e, ref.e)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name}")
    mp, wf, st = r.outputs()
    np.testing.assert_array_equal(mp, ref.mpc_p(), err_msg=f"{what}: mpc_p")
    np.testing.assert_array_equal(st, ref.status(), err_msg=f"{what}: status")
    scale = np.fmax.reduce(np.abs(ref.theta[:, :, 2]), axis=1)[:, None]   # NaN-free where one axis is NaN
    with np.errstate(invalid="ignore"):
        ok = (np.abs(wf - ref.wf) <= 1e-13 * np.abs(ref.wf) + 1e-13 * scale) | (np.isnan(wf) & np.isnan(ref.wf))
    assert ok.all(), (what, np.argwhere(~ok)[:5], np.abs(wf - ref.wf).max())


def run_against_restatement(ba, B, params=None, ticks=300, seed=0):
    p = params if params is not None else ba.RlsParams.default()
    r = ba.BatchRls(B, p)
    ref = RlsffRestatement.from_params(B, p)
    codes = set()
    for k, y, acc, vel, rpy in scenario(B, ticks, seed):
        r.update(y, acc, vel, rpy)
        codes |= set(np.unique(ref.step(y, acc, vel, rpy)).tolist())
        if (k + 1) % 25 == 0:
            assert_matches(r, ref, f"B={B} tick {k}")
    assert_matches(r, ref, f"B={B} end")
    r.close()
    return codes


@pytest.mark.parametrize("B", [1, 63, 65, 4096])
def test_bit_identical_to_restatement(ba, B):
    codes = run_against_restatement(ba, B, seed=B)
    assert codes == {LAM_DOWN, LAM_FLOOR, LAM_UP, LAM_CEIL}, codes   # both lambda branches and both clamps were exercised


@pytest.mark.parametrize("ns,nl", [(3, 17), (1, 1), (50, 256)])
def test_bit_identical_with_other_windows(ba, ns, nl):
    p = ba.RlsParams.default()
    p.n_short, p.n_long = ns, nl
    run_against_restatement(ba, 65, p, seed=100 + nl)


def test_isolation_shuffled_copies(ba):
    """16 384 estimators = a shuffled 32-fold copy of 512: the copies are bit-identical, and equal to the restatement of the 512"""
    Bu, rep = 512, 32
    B = Bu * rep
    perm = np.random.default_rng(9).permutation(B)
    src = perm % Bu                   # instance b of the big batch is a copy of instance src[b]
    r = ba.BatchRls(B)
    ref = RlsffRestatement(Bu)
    for k, y, acc, vel, rpy in scenario(Bu, 120, 17):
        r.update(y[src], acc[src], vel[src], rpy[src])
        ref.step(y, acc, vel, rpy)
    th, P, lam, F, e = r.state()
    mp, wf, st = r.outputs()
    for a, b in ((th, ref.theta), (P, ref.P), (lam, ref.lam), (F, ref.F), (e, ref.e), (mp, ref.mpc_p()), (st, ref.status())):
        np.testing.assert_array_equal(a, b[src])
    for j in range(Bu):
        grp = np.flatnonzero(src == j)
        assert (wf[grp] == wf[grp[0]]).all()
    r.close()


def test_state_round_trip_reset_and_set_state_empties_windows(ba):
    B = 37
    rng = np.random.default_rng(3)
    r = ba.BatchRls(B)
    ref = RlsffRestatement(B)
    th0, P0, lam0, F0, e0 = r.state()
    assert not th0.any() and (lam0 == 0.9).all() and not F0.any() and not e0.any()
    np.testing.assert_array_equal(P0, np.broadcast_to(np.eye(4), (B, 4, 4, 4)))
    gen = scenario(B, 60, 5)
    for k, y, acc, vel, rpy in gen:
        r.update(y, acc, vel, rpy); ref.step(y, acc, vel, rpy)
        if k == 39:
            break
    th = rng.normal(size=(B, 4, 4)); A = rng.normal(size=(B, 4, 4, 4)); P = np.einsum("baij,bakj->baik", A, A) + np.eye(4)
    lam = rng.uniform(0.5, 1.0, (B, 4))
    r.set_state(th, P, lam); ref.set_state(th, P, lam)
    t2, P2, l2, _, _ = r.state()
    np.testing.assert_array_equal(t2, th); np.testing.assert_array_equal(P2, P); np.testing.assert_array_equal(l2, lam)
    for k, y, acc, vel, rpy in gen:   # the windows restart empty: tick 1 after set_state has F = NaN again
        r.update(y, acc, vel, rpy); ref.step(y, acc, vel, rpy)
        if k == 40:
            assert np.isnan(r.state()[3]).all()
    assert_matches(r, ref, "after set_state")
    r.set_state(lam=np.full((B, 4), 0.7))    # one block alone
    assert (r.state()[2] == 0.7).all()
    r.reset()
    th0, P0, lam0, F0, e0 = r.state()
    mp, wf, st = r.outputs()
    assert not th0.any() and (lam0 == 0.9).all() and not F0.any() and not e0.any() and not mp.any() and not wf.any() and not st.any()
    np.testing.assert_array_equal(P0, np.broadcast_to(np.eye(4), (B, 4, 4, 4)))
    ref = RlsffRestatement(B)
    for k, y, acc, vel, rpy in scenario(B, 30, 6):
        r.update(y, acc, vel, rpy); ref.step(y, acc, vel, rpy)
    assert_matches(r, ref, "after reset")
    r.close()


@pytest.mark.parametrize("field,value", [("n_short", 0), ("n_long", 257), ("lambda_min", 0.0), ("lambda0", 1.5), ("lambda0", 0.4),
                                         ("dt", 0.0)])
def test_invalid_params_are_rejected(ba, field, value):
    p = ba.RlsParams.default()
    setattr(p, field, value)
    with pytest.raises(RuntimeError):
        ba.BatchRls(4, p)


def test_batch_mismatch_is_rejected(ba):
    s4 = ba.BatchSolver(4, ba.SolverOptions(10, 0.1))
    e4, e5 = ba.BatchEkf(4), ba.BatchEkf(5)
    r4, r5 = ba.BatchRls(4), ba.BatchRls(5)
    with pytest.raises(RuntimeError):
        r5.update_from_ekf(e4, s4)            # estimator against solver
    with pytest.raises(RuntimeError):
        r4.update_from_ekf(e5, s4)            # estimator against EKF
    with pytest.raises(RuntimeError):
        r5.apply_to_solver(s4)
    with pytest.raises(RuntimeError):
        r4.apply_to_solver(s4, mode=2)
    with pytest.raises(ValueError):
        r4.update(np.zeros((5, 4)), np.zeros((4, 4)), np.zeros((4, 4)), np.zeros((4, 3)))
    for o in (r4, r5, e4, e5, s4):
        o.close()


def test_nan_input_stays_in_its_instance(ba):
    B = 64
    r, clean = ba.BatchRls(B), ba.BatchRls(B)
    ref = RlsffRestatement(B)
    for k, y, acc, vel, rpy in scenario(B, 60, 21):
        clean.update(y, acc, vel, rpy)
        if k == 10:
            y = y.copy(); y[7, 2] = np.nan
        r.update(y, acc, vel, rpy); ref.step(y, acc, vel, rpy)
    _, _, st = r.outputs()
    assert st[7] == 2 and (np.delete(st, 7) == 0).all()
    assert_matches(r, ref, "NaN input")                            # propagated as the reference would
    a, b = r.state(), clean.state()
    keep = np.arange(B) != 7
    for x, y_ in zip(a, b):
        np.testing.assert_array_equal(x[keep], y_[keep])
    np.testing.assert_array_equal(r.outputs()[1][keep], clean.outputs()[1][keep])
    r.close(); clean.close()


def _run_some(ba, r, B, ticks=40):
    ref = RlsffRestatement(B)
    for k, y, acc, vel, rpy in scenario(B, ticks, 33):
        r.update(y, acc, vel, rpy); ref.step(y, acc, vel, rpy)
    return ref


def test_apply_to_solver_disturbance_and_model(ba):
    B, N = 5, 10
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.1))
    rng = np.random.default_rng(8)
    p0 = rng.normal(size=(B, N + 1, 16))
    s.set_params(p0)
    r = ba.BatchRls(B)
    ref = _run_some(ba, r, B)
    r.apply_to_solver(s, ba.APPLY_DISTURBANCE)
    p = s.get_params()
    t2 = ref.theta[:, :, 2]
    want = np.stack([t2[:, 0] / ref.cc, t2[:, 1] / ref.cc, t2[:, 2] / ref.rc, t2[:, 3] / ref.rc], axis=1)
    np.testing.assert_array_equal(p[:, :, :4], np.repeat(want[:, None, :], N + 1, axis=1))
    np.testing.assert_array_equal(p[:, :, 4:], p0[:, :, 4:])
    r.apply_to_solver(s, ba.APPLY_MODEL)
    p = s.get_params()
    np.testing.assert_array_equal(p[:, :, :4], np.repeat(want[:, None, :], N + 1, axis=1))
    for base, comp in ((4, 0), (8, 1), (12, 3)):
        np.testing.assert_array_equal(p[:, :, base:base + 4], np.repeat(ref.theta[:, None, :, comp], N + 1, axis=1))
    r.close(); s.close()


def test_apply_to_solver_leaves_dist6_roll_pitch_alone(ba):
    B, N = 4, 8
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.1))
    s.enable_dist6(True)
    rp = np.random.default_rng(2).normal(size=(B, N + 1, 2))
    s.set_rp_disturbance(rp)
    r = ba.BatchRls(B)
    _run_some(ba, r, B, 20)
    for mode in (ba.APPLY_DISTURBANCE, ba.APPLY_MODEL):
        r.apply_to_solver(s, mode)
        np.testing.assert_array_equal(s.get_rp_disturbance(), rp)
    r.close(); s.close()


def test_device_ampc_loop(ba):
    """the on-device AMPC tick (bluerov2_ampc_node.cpp:28-30): RTI step -> plant step -> EKF from the solver -> RLS from the EKF ->
    p[0..3] of every stage.  Each tick the solver's x0 and the GPU EKF's estimate are read back and the restatement is stepped with
    them: theta and lambda bit-identical every tick (the RLS alone is graded, not the EKF)."""
    B, N = 6, 20
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
    rng = np.random.default_rng(7)
    x0 = np.zeros((B, 12)); x0[:, 2] = -20; x0[:, :2] = rng.uniform(-0.3, 0.3, (B, 2))
    p_true = np.tile(ba.P_NOMINAL, (B, 1)); p_true[:, 0] = rng.uniform(-10, 10, B); p_true[:, 1] = rng.uniform(-10, 10, B)
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(p_true)
    yref = np.zeros((N + 1, 16)); yref[:, 2] = -20
    s.set_yref(yref)
    # the device plant is the OCP model itself: unit scaling of the estimates (see include/bluerov2_nmpc.h)
    pe = ba.EkfParams.default(); pe.compensate_coef = 1.0; pe.rotor_constant = 1.0
    for j in range(12, 24):
        pe.K[j] = 0.0     # the OCP model has no roll / pitch thrust
    e = ba.BatchEkf(B, pe)
    pr = ba.RlsParams.default(); pr.compensate_coef = 1.0; pr.rotor_constant = 1.0
    r = ba.BatchRls(B, pr)
    ref = RlsffRestatement.from_params(B, pr)
    vprev = np.zeros((B, 4))
    for k in range(60):
        s.solve(sync=True)
        s.plant_step(0.05, 1)
        e.update_from_solver(s)
        r.update_from_ekf(e, s)
        r.apply_to_solver(s)
        xs = s.get_x0()
        xe, _ = e.state()
        vel = xs[:, [6, 7, 8, 11]]
        acc = (vel - vprev) / 0.05
        vprev = vel
        ref.step(xe[:, [12, 13, 14, 17]], acc, vel, xs[:, 3:6])
        th, _, lam, _, _ = r.state()
        np.testing.assert_array_equal(th, ref.theta, err_msg=f"tick {k}")
        np.testing.assert_array_equal(lam, ref.lam, err_msg=f"tick {k}")
    _, _, st = r.outputs()
    assert not st.any()
    par = s.get_params()
    np.testing.assert_array_equal(par[:, :, :4], np.repeat(ref.mpc_p()[:, None, :], N + 1, axis=1))
    np.testing.assert_array_equal(par[:, :, 4:], np.tile(ba.P_NOMINAL[4:], (B, N + 1, 1)))
    est = ref.theta[:, :2, 2]
    big = np.abs(p_true[:, :2]) > 3
    assert np.all(np.sign(est[big]) == np.sign(p_true[:, :2][big])), (est, p_true[:, :2])
    r.close(); e.close(); s.close()
