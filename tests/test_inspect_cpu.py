"""The range stage and the inspection controller without a device: known answers of the numpy restatements (tests/inspect_restatement.py),
what the scripted controller sequence of the GPU test covers (tests/inspect_script.py), and the sign of the vertical channel in a CPU loop of
the restated controller and the oracle plant."""
import math

import numpy as np

import inspect_restatement as R
import inspect_script as S
from bluerov2_amd import inspect as I

EYE = np.eye(3).reshape(9)


def _cam(**kw):
    c = I.default_range_params()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_a_face_perpendicular_to_x_at_distance_d():
    for roi, d in ((4, 2.0), (10, 3.5), (40, 1.79)):
        cam = _cam(roi=roi)
        rng, hits, depth = R.cast(EYE, np.zeros(3), cam, [[d, -50.0, -50.0]], [[d + 1.0, 50.0, 50.0]])
        assert hits == roi * roi and np.all(depth == d)
        px = (np.arange(roi) - roi // 2 + 0.5) / cam.f
        fac = np.sqrt(1.0 + px[None, :] ** 2 + px[:, None] ** 2)
        assert abs(rng - d * fac.mean()) <= 4 * roi * roi * np.finfo(float).eps * d     # (the mean in another order of summation)
        assert d < rng < d * 1.002
    # the defaults are the depth sensor's: 1280 pixels over 85.2 degrees
    assert _cam().f == I.range_focal(1280.0, 85.2 * math.pi / 180.0) and abs(_cam().f - 695.99477) < 1e-4


def test_no_return_is_zero_range():
    cam = _cam(roi=10)
    box = ([[2.0, -1.0, -1.0]], [[3.0, 1.0, 1.0]])
    assert R.cast(R.rot_np(0.0, 0.0, math.pi), np.zeros(3), cam, *box)[:2] == (0.0, 0)            # looking away
    assert R.cast(EYE, np.array([1.95, 0.0, 0.0]), cam, *box)[:2] == (0.0, 0)                     # nearer than near
    assert R.cast(EYE, np.array([-99.0, 0.0, 0.0]), cam, *box)[:2] == (0.0, 0)                    # beyond far
    assert R.cast(EYE, np.array([2.5, 0.0, 0.0]), cam, *box)[:2] == (0.0, 0)                      # inside the box
    assert R.cast(EYE, np.zeros(3), cam, np.zeros((0, 3)), np.zeros((0, 3)))[:2] == (0.0, 0)      # no box at all
    r, n, _ = R.cast(EYE, np.zeros(3), cam, *box)
    assert n == 100 and r > 2.0
    # the noise is applied only to a return
    x = np.zeros((2, 12)); x[1, 5] = math.pi
    o = R.range_eval(np.array([EYE, R.rot_np(0, 0, math.pi)]), x, cam, *box, sigma=0.05, m=3)
    assert o["range"][1] == 0.0 and o["hits"][1] == 0 and o["range"][0] != r and abs(o["range"][0] - r) < 0.3


def test_the_grazing_column_is_a_miss_and_nothing_is_nan():
    cam = _cam(roi=4, cx=0.5)
    rng, hits, depth = R.cast(EYE, np.zeros(3), cam, [[2.0, 0.0, -1.0]], [[3.0, 1.0, 1.0]])      # the origin on the face plane y = 0
    d = depth.reshape(4, 4)                                                                      # [j][i], i = -2 ... 1; i = 0 has a = 0
    assert np.all(np.isfinite(depth)) and math.isfinite(rng)
    assert np.all(d[:, :2] == 2.0) and np.all(d[:, 2] == 0.0) and np.all(d[:, 3] == 0.0) and hits == 8


def test_the_scripted_sequence_covers_the_controller():
    par, rng, z, psi = S.sequence()
    states, recs, stats, failed = S.replay(par, rng, z, psi)
    status = states[1:]["status"]
    assert set(np.unique(status)) == {0, 1, 2, 3, 4, 5}
    assert np.all(failed.sum(axis=0) >= 1) and np.array_equal(stats["failed"], failed.sum(axis=0))
    assert np.all(states[-1]["completed_mission"] == 1) and np.all(stats["rounds"] == 2) and np.all(stats["first_done"] > 0)
    assert np.all(states[1]["started"] == 0) and np.all(recs[0]["u0"] == 0.0) and np.all(recs[0]["thrust"] == 0.0)   # before a range is seen
    yaw = np.vectorize(lambda p: math.remainder(p, R.TWO_PI))(psi)
    up = (yaw[:-1] > 2.0) & (yaw[1:] < -2.0)
    down = (yaw[:-1] < -2.0) & (yaw[1:] > 2.0)
    assert np.all(up.sum(axis=0) >= 1) and np.all(down.sum(axis=0) >= 1)                     # +-pi is crossed in both directions
    assert np.all(np.abs(states[-1]["yaw_sum"] - (par.yaw0 + 8 * R.HALF_PI)) < 0.2)          # ... and the unwrapped yaw survives it
    # the record is the solver's: u0 = (c1, c2, -c3, c4), thrust its allocation, status 0
    from bluerov2_amd import thrust_allocation
    assert recs["thrust"].tobytes() == thrust_allocation(recs["u0"]).tobytes() and np.all(recs["status"] == 0)
    # the quirk settings differ
    seen = {}
    for flags in (3, 2, 1, 0):
        q = I.default_inspect_params(); q.flags = flags
        seen[flags] = S.replay(q, rng, z, psi)[1]["u0"]
    for a in seen:
        for b in seen:
            assert a == b or not np.array_equal(seen[a], seen[b]), (a, b)


def test_sign_of_the_vertical_channel(oracle):
    """From depth offsets of +0.5 m and -0.5 m, 200 ticks of the CPU loop (restated controller, oracle plant, the pier in view at the
    stand-off distance) end within 0.5 m of the depth reference; with the sign the wrong way the depth runs away"""
    from bluerov2_amd import P_NOMINAL
    par, cam = I.default_inspect_params(), I.default_range_params()
    for off in (0.5, -0.5):
        for sign in (1.0, -1.0):
            s = I.initial_state(par, 1)
            x = np.zeros(12)
            x[:3], x[5] = [I.START_POSE[0], I.PIER_LO[1] - par.safety_dis, par.z0 + off], par.yaw0
            for k in range(200):
                rng = R.cast(R.rot_np(*x[3:6]), x[:3], cam, [I.PIER_LO], [I.PIER_HI])[0]
                rec, _ = R.control(par, s[0], None, rng, x[2], x[5])
                u = rec["u0"].copy()
                u[1] = 0.0            # (no strafing: the pier stays in view for the whole run)
                u[2] *= sign
                x = oracle.rk4(x, u, P_NOMINAL, par.dt)
                if abs(x[2] - par.z0) > 50.0:
                    break
            print(f"offset {off:+.1f} sign {sign:+.0f}: z - z0 = {x[2] - par.z0:+.4f} after {k + 1} ticks")
            if sign > 0:
                assert abs(x[2] - par.z0) < 0.5, (off, x[2] - par.z0)
            else:
                assert abs(x[2] - par.z0) > 5.0, (off, x[2] - par.z0)
