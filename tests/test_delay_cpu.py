"""The delay stage without a GPU: the numpy restatement (tests/delay_restatement.py) against answers worked by hand, and the ordering of the
CPU loop that the device test asserts again -- a 2-tick input delay hurts the shipped controller, predicting through it repairs most of it."""
import numpy as np
import pytest

from oracle import trajectory_oracle as T
from delay_restatement import DelayRestatement, cpu_delay_loop, rms_position_error


def _commands(n, B=2):
    """distinct dyadic commands of step n: u0[b] = (n + 1 + 16 b) * (1, -1, 0.5, 0.25), thrust[b] = 100 (n + 1) + b + (0, 0.125, ..., 0.625)"""
    s = (n + 1 + 16.0 * np.arange(B))[:, None]
    return s * np.array([1.0, -1.0, 0.5, 0.25]), 100.0 * (n + 1) + np.arange(B)[:, None] + 0.125 * np.arange(6)[None, :]


def test_restatement_has_the_answers_worked_by_hand():
    """B = 2, delays (0, 2), five steps.  Instance 0 is applied what is commanded.  Instance 1 gets zeros on steps 0 and 1, then the commands of
    steps 0, 1, 2.  D = 3: the queue holds the last three commands oldest first, zeros where there was no step yet."""
    r = DelayRestatement(2, delay=[0, 2])
    assert r.D == 3 and r.n == 0 and not r.queue().any()
    au0, at0, q0 = [], [], []
    for n in range(5):
        u0, t = _commands(n)
        au, at = r.step(u0, t)
        au0.append(au); at0.append(at); q0.append(r.queue())
    au0, at0 = np.array(au0), np.array(at0)
    # first components, written out: commanded u0[0] is 1, 2, 3, 4, 5 (instance 0) and 17, 18, 19, 20, 21 (instance 1)
    assert np.array_equal(au0[:, 0, 0], [1.0, 2.0, 3.0, 4.0, 5.0])
    assert np.array_equal(au0[:, 1, 0], [0.0, 0.0, 17.0, 18.0, 19.0])
    assert np.array_equal(at0[:, 0, 0], [100.0, 200.0, 300.0, 400.0, 500.0])
    assert np.array_equal(at0[:, 1, 5], [0.0, 0.0, 101.625, 201.625, 301.625])
    # whole records
    for n in range(5):
        u0, t = _commands(n)
        assert np.array_equal(au0[n, 0], u0[0]) and np.array_equal(at0[n, 0], t[0])
        if n < 2:
            assert not au0[n, 1].any() and not at0[n, 1].any()                      # zeros before the first delivery
        else:
            u0d, td = _commands(n - 2)
            assert np.array_equal(au0[n, 1], u0d[1]) and np.array_equal(at0[n, 1], td[1])
    # the queue, oldest first
    assert np.array_equal(q0[0][:, :, 0], [[0.0, 0.0, 1.0], [0.0, 0.0, 17.0]])
    assert np.array_equal(q0[1][:, :, 0], [[0.0, 1.0, 2.0], [0.0, 17.0, 18.0]])
    assert np.array_equal(q0[4][:, :, 0], [[3.0, 4.0, 5.0], [19.0, 20.0, 21.0]])
    assert np.array_equal(q0[4][1, :, 3], [0.25 * 19, 0.25 * 20, 0.25 * 21])
    assert r.n == 5 and np.array_equal(r.last[:, :4], au0[4])
    r.reset()
    assert r.n == 0 and not r.queue().any() and not r.ring.any()


def test_depth_covers_the_predictor_and_its_inputs_are_the_last_commands():
    """D = max(max delay, comp) + 1; the predictor integrates through the last comp commanded u0, zeros for steps before the first"""
    assert DelayRestatement(3, delay=[0, 1, 2], comp=0).D == 3 and DelayRestatement(3, delay=0, comp=4).D == 5 and DelayRestatement(1).D == 1
    r = DelayRestatement(2, delay=[0, 2], comp=3)
    assert r.D == 4 and r.predictor_inputs().shape == (3, 2, 4) and not r.predictor_inputs().any()
    r.step(*_commands(0))
    assert np.array_equal(r.predictor_inputs()[:, :, 0], [[0.0, 0.0], [0.0, 0.0], [1.0, 17.0]])
    for n in range(1, 6):
        r.step(*_commands(n))
    assert np.array_equal(r.predictor_inputs()[:, :, 0], [[4.0, 20.0], [5.0, 21.0], [6.0, 22.0]])
    assert np.array_equal(r.queue()[:, :, 0], [[3.0, 4.0, 5.0, 6.0], [19.0, 20.0, 21.0, 22.0]])
    with pytest.raises(AssertionError):
        DelayRestatement(2, delay=[0, 9])


def test_prediction_repairs_most_of_what_a_two_tick_delay_costs(oracle):
    """N = 20, B = 4, seed 21, the circle, 40 ticks (scripts/delay_cpu_scenarios.py; DESIGN.md section 4.9e has 0.077 m undelayed, 0.377 m
    with a 2-tick delay, 0.106 m with the delay predicted through).  The bounds are the issue's: the compensated loop is below half the
    uncompensated one's error and below twice the undelayed loop's; every step succeeds."""
    from bluerov2_amd.solver import P_NOMINAL
    N, B, ticks = 20, 4, 40
    rng = np.random.default_rng(21)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
    pp = np.tile(P_NOMINAL, (B, 1))
    rms = {}
    for name, delay, comp in (("none", 0, 0), ("delayed", 2, 0), ("predicted", 2, 2)):
        log = cpu_delay_loop(oracle, DelayRestatement(B, delay, comp), traj, x0, P_NOMINAL, pp, N, ticks)
        assert log["x"].shape == (ticks + 1, B, 12) and np.isfinite(log["x"]).all() and not log["status"].any(), name
        rms[name] = rms_position_error(log["x"], traj)
    print("RMS position error over 40 ticks: " + ", ".join(f"{k} {v:.4f} m" for k, v in rms.items()))
    assert rms["predicted"] < 0.5 * rms["delayed"]
    assert rms["predicted"] < 2.0 * rms["none"]
