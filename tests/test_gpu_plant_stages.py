"""GPU test of the solver's plant with ALL its stages on at once -- a periodic world wrench, the thruster stage with limits and a fault, the
sensor stage with noise, bias, a period and dropout -- which no other test does: brov_closed_loop_ex and brov_closed_loop_dob from a seeked
tick counter against a second solver driven through the public calls, tick by tick.  Both sides are the library itself: every comparison is
exact.  B = 3, N = 10, 6 ticks of 2 substeps, 16-column windows."""
import numpy as np
import pytest

from oracle import trajectory_oracle as T

pytestmark = pytest.mark.gpu
B, N, TICKS, SUBSTEPS, LINE0, SEEK = 3, 10, 6, 2, 1, 5
PERIODIC = dict(seed=0xB10E, scale=6.0, phase0=0.25, dphi=0.125, tz_div=3.0)


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


@pytest.fixture(scope="module")
def start():
    """(trajectory, start states near its first row), shared and left unchanged"""
    rng = np.random.default_rng(41)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
    for a in (traj, x0):
        a.setflags(write=False)
    return traj, x0


def _solver(ba, start):
    """a solver with the three stages on, its counter at SEEK"""
    traj, x0 = start
    rng = np.random.default_rng(42)
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(np.tile(ba.P_NOMINAL, (B, 1))); s.set_trajectory(traj)
    s.set_plant_wrench(periodic=PERIODIC)
    s.plant_wrench_seek(SEEK)
    # instance 1: a weak thruster from tick 2 of the counter on (every tick of the run); instance 0: another from the run's own tick 2 on
    gain = np.ones((B, 6)); gain[1, 2] = 0.5; gain[0, 4] = 0.75
    s.set_thrusters(lo=-30.0, hi=30.0, gain=gain, onset=np.array([SEEK + 2, 2, 0]))
    period = np.ones(12, dtype=np.int32); period[5] = 2
    dropout = np.zeros(B); dropout[2] = 0.5
    s.set_sensors(seed=0x5EA5, sigma=rng.uniform(0.001, 0.02, (B, 12)), bias=rng.uniform(-0.01, 0.01, (B, 12)), period=period, dropout=dropout)
    return s


def _ekf(ba):
    """the observer configured for the device plant, as tests/test_gpu_sensors.py::_ekf does"""
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
    return ba.BatchEkf(B, par)


def _end(s):
    """what a run leaves behind in the plant and its stages"""
    th, sn = s.thruster_stats(), s.sensor_stats()
    return dict(x=s.get_x0(), y=s.measured_state(), tick=s.plant_wrench_tick(), clip_ticks=th["clip_ticks"], lost_sq=th["lost_sq"],
                steps=th["steps"], dropped=sn["dropped"], err_sq=sn["err_sq"], refreshes=sn["refreshes"], results=s.results().tobytes())


def _by_calls(s, e):
    """the loop through the public calls, tick by tick; the wrench of a tick from the generator at the counter's value"""
    log = dict(u=[], x=[s.get_x0()], status=[], wrench=[], est=[])
    for k in range(TICKS):
        s.set_yref_from_trajectory(LINE0 + k, 16); s.solve()
        log["wrench"].append(s.plant_wrench(s.plant_wrench_tick()))
        s.plant_step(0.05, SUBSTEPS)
        if e is not None:
            e.update_from_solver(s); e.apply_to_solver(s)
            log["est"].append(e.state()[0][:, 12:].copy())
        res = s.results()
        log["u"].append(res["u0"].copy()); log["status"].append(res["status"].copy()); log["x"].append(s.get_x0())
    return {k: np.array(v) for k, v in log.items() if len(v)}


def _same_end(a, b):
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert a["tick"] == SEEK + TICKS == 11 and a["steps"] == TICKS and a["refreshes"] == TICKS


def test_closed_loop_with_every_stage_on_equals_its_call_sequence(ba, start):
    a, b = _solver(ba, start), _solver(ba, start)
    ul, xl, sl, wl = a.closed_loop(TICKS, line0=LINE0, dt=0.05, substeps=SUBSTEPS, log_wrench=True)
    assert a.last_kernel_path() == ba.PATH_FUSED
    # no stage is plain: a launch per step, so the window in force is none that brov_set_yref_from_traj built (the one-launch form leaves one)
    with pytest.raises(RuntimeError, match="brov_solve_ticks: a moving window"):
        a.solve_ticks(1, row_stride=1)
    seq = _by_calls(b, None)
    for key, got in (("u", ul), ("x", xl), ("status", sl), ("wrench", wl)):
        assert np.array_equal(got, seq[key]), key
    ea, eb = _end(a), _end(b)
    _same_end(ea, eb)
    assert np.array_equal(ea["x"], xl[-1]) and np.abs(ea["y"] - ea["x"]).max() > 1e-4          # the true state; the measurement is not it
    assert np.abs(wl).max() > 0.1 and ea["lost_sq"][1] > 0.0 and ea["err_sq"].min() > 0.0      # every stage was felt
    # every stage off: the same call takes the one-launch form again at this horizon, and leaves the stages' counts alone
    a.thrusters_off(); a.sensors_off(); a.plant_wrench_off()
    a.closed_loop(TICKS, line0=LINE0, dt=0.05, substeps=SUBSTEPS)
    assert a.last_kernel_path() == ba.PATH_FUSED and a.plant_wrench_tick() == SEEK + 2 * TICKS
    assert a.thruster_stats()["steps"] == TICKS and a.sensor_stats()["refreshes"] == TICKS
    a.solve_ticks(1, row_stride=1, sync=True)                          # (the window in force names rows of the table)
    a.close(); b.close()


def test_dob_loop_with_every_stage_on_equals_its_five_calls(ba, start):
    a, ea, b, eb = _solver(ba, start), _ekf(ba), _solver(ba, start), _ekf(ba)
    log = a.closed_loop_dob(ea, ticks=TICKS, line0=LINE0, dt=0.05, substeps=SUBSTEPS)
    assert a.last_kernel_path() == ba.PATH_FUSED
    seq = _by_calls(b, eb)
    assert set(seq) == set(log)
    for key in seq:
        assert np.array_equal(log[key], seq[key]), key
    _same_end(_end(a), _end(b))
    assert np.array_equal(a.get_params(), b.get_params())
    for p, q in zip(ea.state(), eb.state()):
        assert np.array_equal(p, q)
    assert np.abs(log["est"]).max() > 0.0
    for o in (a, ea, b, eb):
        o.close()
