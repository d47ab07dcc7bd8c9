"""The range stage and the inspection controller on the device (brov_range_*, brov_inspect_*, brov_closed_loop_inspect), B = 5, N = 20,
against tests/inspect_restatement.py.

Bars.  The rotation the rays are cast with against a 60-digit (mpmath) one: a scaled error <= 4 x max(E_np, 2^-50), the suite's own
(tests/test_gpu_eskf_exact.py), E_np the error of the numpy rotation against the same 60-digit values, computed here.  Everything else --
per-ray depths, hits, the mean range with and without noise, the controller's state, record and statistics, the logs of the loop -- bit for bit."""
import numpy as np
import pytest

import inspect_restatement as R
import inspect_script as S
from bluerov2_amd import inspect as I

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2.0 ** -50
B, N, DT = 5, 20, 0.05
ERR_ARG = -1
PIER = (np.array([I.PIER_LO]), np.array([I.PIER_HI]))


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


def _solver(ba, batch=B):
    s = ba.BatchSolver(batch, ba.SolverOptions(N, DT), device=0)
    yref = np.zeros((N + 1, 16)); yref[:, :3] = [2.0, 0.0, -20.0]
    x0 = np.zeros((batch, 12)); x0[:, :3] = [2.0, 0.0, -20.0]
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_yref(yref)
    return s


@pytest.fixture(scope="module")
def solver(ba):
    s = _solver(ba)
    yield s
    s.close()


def _poses(batch=B):
    """x [batch, 12] and the boxes: a wall whose face x = 2 is perpendicular to body x at zero attitude, seen from the origin"""
    x = np.zeros((batch, 12))
    x[0, :3] = [0.0, 0.0, 0.0]                                   # facing the face at 2 m
    x[1, :3] = [0.0, 1.0, 0.0]                                   # straddling the edge y = 1
    x[2, :3], x[2, 5] = [0.0, 0.0, 0.0], np.pi                   # looking away
    x[3, :3] = [1.95, 0.0, 0.0]                                  # too near: 0.05 < near
    x[4, :3], x[4, 3], x[4, 4] = [0.3, -0.2, 0.1], 0.3, 0.3      # rolled and pitched
    for b in range(5, batch):
        x[b, :3], x[b, 3:6] = [0.1 * (b % 7), 0.05 * (b % 5), 0.0], [0.01 * b, -0.02 * (b % 9), 0.3 * (b % 4)]
    lo = np.array([[2.0, -1.0, -1.5], [-9.0, 4.0, -1.0], [2.5, -3.0, -0.2], [0.0, 0.0, 60.0], [-50.0, -1.0, -1.0], [2.2, 0.5, 0.5],
                   [3.0, -8.0, -8.0], [-1.0, -1.0, -30.0]])
    hi = np.array([[3.0, 1.0, 1.5], [-8.0, 5.0, 1.0], [2.6, 3.0, 0.2], [1.0, 1.0, 61.0], [-49.0, 1.0, 1.0], [2.4, 0.9, 0.9],
                   [3.5, 8.0, 8.0], [1.0, 1.0, -29.0]])
    return x, lo, hi


def _rot_ok(rot, x):
    worst = 0.0
    for b in range(len(x)):
        e_np = R.rot_error(R.rot_np(*x[b, 3:6]), *x[b, 3:6])
        e_dev = R.rot_error(rot[b], *x[b, 3:6])
        print(f"rot instance {b}: device {e_dev:.3e} numpy {e_np:.3e} ratio {e_dev / max(e_np, FLOOR):.2f}")
        assert e_dev <= FACTOR * max(e_np, FLOOR), (b, e_dev, e_np)
        worst = max(worst, e_dev / max(e_np, FLOOR))
    return worst


@pytest.mark.parametrize("roi", [4, 10, 40])
@pytest.mark.parametrize("K", [1, 2, 8])
def test_range_alone_bit_for_bit(ba, solver, roi, K):
    s = solver
    x, lo, hi = _poses()
    s.set_range_scene(lo[:K], hi[:K])
    s.set_range(roi=roi, seed=11)
    cam = I.default_range_params(); cam.roi, cam.seed = roi, 11
    o = s.range_eval(7, x, rot=True, depth=True)
    _rot_ok(o["rot"], x)
    r = R.range_eval(o["rot"], x, cam, lo[:K], hi[:K], m=7)
    assert np.array_equal(o["hits"], r["hits"]), (o["hits"], r["hits"])
    assert o["depth"].tobytes() == r["depth"].tobytes(), np.abs(o["depth"] - r["depth"]).max()
    assert o["range"].tobytes() == r["range"].tobytes(), (o["range"], r["range"])
    assert o["hits"][0] == roi * roi and np.all(o["depth"][0] == 2.0)
    if K <= 2:                                                                 # (the eight boxes put something behind every pose)
        assert o["hits"][2] == 0 and o["range"][2] == 0.0 and 0 < o["hits"][1] < roi * roi          # looking away; straddling the edge
    if K == 1:
        assert o["hits"][3] == 0 and o["range"][3] == 0.0                      # nearer than near
    again = s.range_eval(7, x, rot=True, depth=True)
    assert all(o[k].tobytes() == again[k].tobytes() for k in o)
    # with noise
    sigma = 0.01 * (1 + np.arange(B))
    s.set_range(roi=roi, seed=11, sigma=sigma)
    n = s.range_eval(9, x)
    rn = R.range_eval(o["rot"], x, cam, lo[:K], hi[:K], sigma=sigma, m=9)
    assert n["range"].tobytes() == rn["range"].tobytes() and np.array_equal(n["hits"], o["hits"])
    assert np.all((n["range"] != o["range"]) == (o["hits"] > 0))


def test_range_too_far_and_grazing(ba, solver):
    s = solver
    x = np.zeros((B, 12))
    lo, hi = np.array([[2.0, 0.0, -1.0]]), np.array([[3.0, 1.0, 1.0]])       # the origin lies on the face plane y = 0
    s.set_range_scene(lo, hi)
    s.set_range(roi=4, cx=0.5, far=1.5)
    cam = I.default_range_params(); cam.roi, cam.cx, cam.far = 4, 0.5, 1.5
    o = s.range_eval(0, x, rot=True, depth=True)
    assert np.all(o["hits"] == 0) and np.all(o["range"] == 0.0)                # beyond far
    s.set_range(roi=4, cx=0.5)
    cam.far = 100.0
    o = s.range_eval(0, x, rot=True, depth=True)
    r = R.range_eval(o["rot"], x, cam, lo, hi)
    assert o["depth"].tobytes() == r["depth"].tobytes() and o["range"].tobytes() == r["range"].tobytes() and np.array_equal(o["hits"], r["hits"])
    d = o["depth"][0].reshape(4, 4)                                            # [j][i]: i = 0 is the grazing column (a = 0, D_y = -0)
    assert np.all(d[:, 2] == 0.0) and np.all(np.isfinite(o["depth"])) and np.all(np.isfinite(o["range"]))
    assert np.all(d[:, :2] == 2.0) and np.all(d[:, 3] == 0.0) and o["hits"][0] == 8


def test_range_does_not_depend_on_the_batch(ba, solver):
    x69, lo, hi = _poses(69)
    s69 = _solver(ba, 69)
    try:
        for s in (solver, s69):
            s.set_range_scene(lo, hi)
        solver.set_range(roi=10, seed=3, sigma=0.02)
        s69.set_range(roi=10, seed=3, sigma=0.02)
        a = solver.range_eval(5, x69[:B], rot=True, depth=True)
        b = s69.range_eval(5, x69, rot=True, depth=True)
        assert all(a[k].tobytes() == b[k][:B].tobytes() for k in a)
    finally:
        s69.close()


@pytest.mark.parametrize("flags", [3, 0, 1, 2])
def test_controller_alone_bit_for_bit(ba, solver, flags):
    s = solver
    par, rng, z, psi = S.sequence()
    par.flags = flags
    s.set_inspect(par)
    try:
        states, recs, stats, _ = S.replay(par, rng, z, psi)
        st, t = I.initial_state(par, B), I.initial_stats(B)
        for k in range(len(rng)):
            st, rec, t = s.inspect_eval(st, rng[k], z[k], psi[k], stats=t)
            assert R.same_bytes(st, states[k + 1]), (k, st, states[k + 1])
            assert R.same_bytes(rec, recs[k]), (k, rec, recs[k])
            assert rec["thrust"].tobytes() == ba.thrust_allocation(rec["u0"]).tobytes(), k
        assert R.same_bytes(t, stats), (t, stats)
        assert np.all(rec["status"] == 0) and np.all(rec["cost"] == 0) and np.all(rec["qp_iter"] == 0)
    finally:
        s.inspect_off()


def _pier_start(batch=B):
    x = np.zeros((batch, 12))
    x[:, :3], x[:, 5] = I.START_POSE[:3], I.START_POSE[3]
    x[:, 0] += 0.03 * np.arange(batch); x[:, 2] += 0.1 * np.arange(batch) - 0.2; x[:, 5] += 0.02 * np.arange(batch)
    return x


def _behind_the_plant(ba, s, ticks, seen):
    """teacher-forced: every tick the restatement is fed the device's state, true for the range and `seen()` for z and psi"""
    par, cam = I.default_inspect_params(), I.default_range_params()
    cam.seed = 5
    st, t = I.initial_state(par, B), I.initial_stats(B)
    for k in range(ticks):
        x_true, y = s.get_x0(), seen()
        m = int(s._L.brov_plant_wrench_tick(s._h))
        s.inspect_step()
        dev_state, dev_range = s.inspect_state()
        rot = s.range_eval(m, x_true, rot=True)["rot"]
        r = R.range_eval(rot, x_true, cam, *PIER, sigma=0.01, m=m)
        assert dev_range.tobytes() == r["range"].tobytes(), (k, dev_range, r["range"])
        st, rec, t, _ = R.control_batch(par, st, t, r["range"], y[:, 2], y[:, 5])
        assert R.same_bytes(dev_state, st), (k, dev_state, st)
        assert R.same_bytes(s.results(), rec), (k, s.results(), rec)
        s.plant_step(DT, 2)
    assert R.same_bytes(s.inspect_stats(), t)
    assert np.all(st["started"] == 1)


def _fresh(ba):
    s = _solver(ba)
    s.set_x0(_pier_start())
    s.set_range_scene(*PIER)
    s.set_range(sigma=0.01, seed=5)
    return s


def test_behind_the_plant_plain(ba):
    s = _fresh(ba)
    try:
        s.set_inspect()
        _behind_the_plant(ba, s, 30, s.get_x0)
    finally:
        s.close()


def test_behind_the_plant_with_thrusters_and_a_current(ba):
    s = _fresh(ba)
    try:
        s.set_thrusters(lo=np.full(6, -30.0), hi=np.full(6, 30.0))
        s.set_current(constant=[0.1, -0.05, 0.0])
        s.set_inspect()
        _behind_the_plant(ba, s, 30, s.get_x0)
    finally:
        s.close()


def test_behind_the_plant_with_the_sensor_stage(ba):
    s = _fresh(ba)
    try:
        s.set_sensors(seed=9, sigma=0.01)
        s.set_inspect()
        _behind_the_plant(ba, s, 30, s.measured_state)
        assert not np.array_equal(s.measured_state(), s.get_x0())
    finally:
        s.close()


def test_loop_equals_the_composed_calls(ba):
    a, b = _fresh(ba), _fresh(ba)
    try:
        ticks = 25
        for s in (a, b):
            s.set_rotors(tau=0.1, h=DT)
            s.set_inspect()
        ul, xl, sl, rl = a.closed_loop_inspect(ticks, DT, 2)
        x = [b.get_x0()]
        u, st, r = [], [], []
        for k in range(ticks):
            b.inspect_step()
            state, rng = b.inspect_state()
            u.append(b.results()["u0"].copy()); st.append(state["status"].copy()); r.append(rng)
            b.plant_step(DT, 2)
            x.append(b.get_x0())
        assert xl.tobytes() == np.array(x).tobytes() and ul.tobytes() == np.array(u).tobytes()
        assert sl.tobytes() == np.array(st, dtype=np.int32).tobytes() and rl.tobytes() == np.array(r).tobytes()
        assert R.same_bytes(a.inspect_stats(), b.inspect_stats()) and R.same_bytes(a.inspect_state()[0], b.inspect_state()[0])
        # the statistics are the restatement's over the logged run (z and psi are the true state's here)
        par = I.default_inspect_params()
        s0, t = I.initial_state(par, B), I.initial_stats(B)
        for k in range(ticks):
            s0, _, t, _ = R.control_batch(par, s0, t, rl[k], xl[k][:, 2], xl[k][:, 5])
        assert R.same_bytes(a.inspect_stats(), t)
        assert np.any(rl > 0)
    finally:
        a.close(); b.close()


def test_refusals_and_neighbours(ba):
    s = _solver(ba)
    L = s._L
    err = lambda: L.brov_last_error().decode()   # noqa: E731
    try:
        # a solver on which the feature was never set: what it solves and steps to (the second of two runs from the same start, so that
        # whatever a solve keeps of the one before it is the same every time)
        it0 = s.get_iterate()
        x0 = np.zeros((B, 12)); x0[:, :3] = [2.0, 0.0, -20.0]

        def again():
            for _ in range(2):
                s.set_iterate(*it0); s.set_x0(x0); s.plant_wrench_seek(0)
                s.solve(sync=True)
                r = s.results().copy()
                s.plant_step(DT, 1)
            return r, s.get_x0()
        rec0, x1 = again()
        r, x = again()
        assert r.tobytes() == rec0.tobytes() and x.tobytes() == x1.tobytes()
        # the controller on, no scene: a step is refused
        s.set_inspect()
        assert L.brov_inspect_step(s._h, None) == ERR_ARG and err().startswith("brov_inspect_step: the scene has no box")
        assert L.brov_closed_loop_inspect(s._h, 3, DT, 1, None, None, None, None) == ERR_ARG and err().startswith("brov_closed_loop_inspect:")
        s.set_range_scene(*PIER)
        assert L.brov_closed_loop_inspect(s._h, 3, 0.04, 1, None, None, None, None) == ERR_ARG and "dt is not its period" in err()
        assert L.brov_plant_step(s._h, 0.04, 1, None) == ERR_ARG and err().startswith("brov_plant_step")
        s.set_delay(np.ones(B, dtype=np.int32), comp=1)
        assert L.brov_inspect_step(s._h, None) == ERR_ARG and "comp > 0" in err()
        assert L.brov_closed_loop_inspect(s._h, 3, DT, 1, None, None, None, None) == ERR_ARG and "comp > 0" in err()
        s.delay_off()
        s.plant_wrench_seek((1 << 24) - 2)
        assert L.brov_closed_loop_inspect(s._h, 3, DT, 1, None, None, None, None) == ERR_ARG and "[0, 2^24)" in err()
        s.plant_wrench_seek(0)
        # the fleet refuses the solver
        f = ba.Fleet(s, 1)
        try:
            assert f._L.brov_fleet_step(f._h, None, DT, 1, None) == ERR_ARG
            assert "inspection controller" in f._L.brov_fleet_last_error().decode()
        finally:
            f.close()
        s.inspect_step()
        assert not np.array_equal(s.results()["u0"], rec0["u0"])
        # off again: the solver solves and steps to the bytes it gave before
        s.inspect_off()
        assert not s.inspect_enabled()
        assert L.brov_inspect_step(s._h, None) == ERR_ARG and "controller is off" in err()
        r, x = again()
        assert r.tobytes() == rec0.tobytes() and x.tobytes() == x1.tobytes()
        assert s.plant_step(0.04, 1) is None
    finally:
        s.close()
