"""GPU tests of the sensor stage (brov_sensor_*, sensor_measure_kernel, sensor_eval_kernel) against tests/sensor_restatement.py and against
twin solvers that never had the stage.  B = 130 is two blocks of the kernels and a ragged tail; every comparison is exact."""
import numpy as np
import pytest

from oracle import trajectory_oracle as T
from sensor_restatement import SensorRestatement, same, same_stats

pytestmark = pytest.mark.gpu
B, N = 130, 10
SEED = 0x5EA5CAFE0123
PERIOD = [1, 1, 1, 2, 2, 3, 1, 1, 1, 2, 2, 3]


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


@pytest.fixture(scope="module")
def start():
    """(trajectory, start states near its first row, plant parameters), shared and left unchanged"""
    import bluerov2_amd as ba
    rng = np.random.default_rng(31)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = rng.uniform(-20, 20, (B, 4))
    for a in (traj, x0, pp):
        a.setflags(write=False)
    return traj, x0, pp


def _config(periods=True):
    """noise, bias, quantisation of four channels, periods, dropout 0.35 on the odd instances"""
    rng = np.random.default_rng(32)
    sigma = rng.uniform(0.0, 0.02, (B, 12)); sigma[3] = 0.0
    bias = rng.uniform(-0.01, 0.01, (B, 12)); bias[:, 2] = 0.05                   # a depth-sensor bias
    quant = np.zeros(12); quant[[0, 1, 2, 5]] = [0.01, 0.01, 0.0078125, 0.001]
    dropout = np.where(np.arange(B) % 2 == 1, 0.35, 0.0)
    return dict(seed=SEED, sigma=sigma, bias=bias, quant=quant, period=PERIOD if periods else None, dropout=dropout)


def _solver(ba, start):
    traj, x0, pp = start
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(pp); s.set_trajectory(traj)
    return s


def _ekf(ba):
    """the observer configured for the device plant, as tests/test_gpu_plant_wrench.py::_ekf_pair does"""
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
    return ba.BatchEkf(B, par)


def _rls(ba):
    rp = ba.RlsParams.default(); rp.compensate_coef = 1.0; rp.rotor_constant = 1.0
    return ba.BatchRls(B, rp)


# ---- 1. the stage alone, bit for bit ----------------------------------------------------------------------------------------------------------
def test_stage_alone_matches_the_restatement_bit_for_bit(ba):
    rng = np.random.default_rng(33)
    x = rng.normal(size=(B, 12)) * 3.0
    x[0, 0] = np.nan; x[129, 11] = np.nan; x[1, 1] = 0.0; x[2, 2] = -0.0; x[3, 5] = 1e6; x[128, 0] = -1e6; x[129, 2] = 1e6
    cfg = _config()
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    assert not s.sensors_enabled()
    s.set_sensors(**cfg)
    assert s.sensors_enabled()
    r = SensorRestatement(B, **cfg)
    y_before = s.measured_state()
    seen = set()
    for m in (0, 1, 77, 2 ** 24 - 1):
        y, dr = s.sensor_eval(m, x)
        assert same(y, r.sample(m, x)), m
        assert np.array_equal(dr, r.verdict(m).astype(np.int32)), m
        assert not dr[::2].any()                                       # dropout 0 never drops
        seen.add(y[~np.isnan(y)].tobytes())
    assert len(seen) == 4 and 0 < dr.sum() < B // 2                    # every index draws afresh
    assert np.isnan(y[0, 0]) and np.isnan(y[129, 11]) and np.isnan(y).sum() == 2
    q = cfg["quant"]
    for c in (0, 1, 2, 5):                                             # quantised channels are multiples of their step (exact for dyadic 2^-7)
        ok = ~np.isnan(y[:, c])
        assert np.abs(y[ok, c] / q[c] - np.rint(y[ok, c] / q[c])).max() < 1e-6
    for bad in (2 ** 24, -1):
        with pytest.raises(RuntimeError, match="brov_sensor_eval_host: the sensor stage's measurement index"):
            s.sensor_eval(bad, x)
    # evaluation moves nothing
    st = s.sensor_stats()
    assert st["refreshes"] == 0 and not st["dropped"].any() and not st["err_sq"].any() and s.plant_wrench_tick() == 0
    assert np.array_equal(s.measured_state(), y_before)
    s.close()


# ---- 2. plant steps: regular refreshes, statistics, and the true state untouched ----------------------------------------------------------------
def test_plant_steps_refresh_the_measurement_and_leave_the_true_state_alone(ba, start):
    traj, x0, _ = start
    cfg = _config()
    s, twin = _solver(ba, start), _solver(ba, start)
    for o in (s, twin):
        o.set_yref(traj[:N + 1]); o.solve()
    s.set_sensors(**cfg)
    r = SensorRestatement(B, **cfg)
    r.forced(0, x0)
    assert same(s.measured_state(), r.y) and same_stats(s.sensor_stats(), r)      # the forced refresh of set_sensors, no statistic
    drops = []
    for k in range(7):
        s.plant_step(0.05, 1); twin.plant_step(0.05, 1)
        x = s.get_x0()
        assert np.array_equal(x, twin.get_x0()), k                     # the plant does not see the stage
        drops.append(r.refresh(k + 1, x))
        assert same(s.measured_state(), r.y), k
        assert same_stats(s.sensor_stats(), r), k
    assert s.plant_wrench_tick() == 7 and r.refreshes == 7
    drops = np.array(drops)
    assert (drops.any(0) & ~drops.all(0)).any()                        # some instance shows a dropped and a taken fix
    assert not drops[:, ::2].any() and r.err_sq.min() > 0.0
    # a held channel is stale: on the even instances (which drop nothing) channel 5 (period 3) still holds the sample of index 6 at index 7,
    # channel 0 (period 1) is the fresh sample
    fresh7 = r.sample(7, x)
    assert np.array_equal(r.y[::2, 0], fresh7[::2, 0]) and (r.y[::2, 5] != fresh7[::2, 5]).mean() > 0.5
    s.close(); twin.close()


# ---- 3. the solve reads the measurement -------------------------------------------------------------------------------------------------------
def test_the_solve_reads_the_measurement_and_a_tick_with_x0_reads_its_own(ba, start, monkeypatch):
    traj, x0, _ = start
    cfg = _config()
    rng = np.random.default_rng(34)
    x = x0 + rng.normal(size=(B, 12)) * 0.01
    s, twin = _solver(ba, start), _solver(ba, start)
    for o in (s, twin):
        o.set_yref(traj[:N + 1])
    s.set_sensors(**cfg)
    r = SensorRestatement(B, **cfg)
    s.set_x0(x); s.solve(sync=True)
    y = r.forced(0, x)
    assert same(s.measured_state(), y) and np.array_equal(s.get_x0(), x) and np.abs(y - x).max() > 1e-3
    twin.set_x0(y); twin.solve(sync=True)
    ra, rb = s.results(), twin.results()
    assert ra.tobytes() == rb.tobytes() and np.all(ra["status"] == 0)
    # a tick that brings its own x0 is solved at that x0: the caller supplied the measurement
    ta, tb = s.tick(x0=x), twin.tick(x0=x)
    assert ta.tobytes() == tb.tobytes() and ta.tobytes() != ra.tobytes()
    # ... also when the tick copies its x0 into the device array ahead of the launch instead of having the kernel read it in place
    monkeypatch.setenv("BROV_TICK_ZEROCOPY", "0")
    s.reload_knobs(); twin.reload_knobs()
    x2 = x0 + rng.normal(size=(B, 12)) * 0.01
    ta, tb = s.tick(x0=x2), twin.tick(x0=x2)
    assert ta.tobytes() == tb.tobytes() and np.array_equal(s.get_x0(), x2)
    s.close(); twin.close()


# ---- 4. neutral wiring ------------------------------------------------------------------------------------------------------------------------
def test_a_neutral_stage_is_the_loop_without_it(ba, start):
    """all zeros, period 1, dropout 0: the measured state is the true state, so the loop with the stage equals the loop without, tick for
    tick.  Both run under a constant zero world wrench, which puts both on the launch-per-tick form."""
    out = []
    for on in (True, False):
        s = _solver(ba, start)
        s.set_plant_wrench(constant=np.zeros(6))
        if on:
            s.set_sensors()
        ul, xl, sl = s.closed_loop(6, line0=2)
        if on:
            assert np.array_equal(s.measured_state(), s.get_x0()) and not s.sensor_stats()["err_sq"].any()
            assert s.sensor_stats()["refreshes"] == 6
        out.append((ul, xl, sl, s.results().tobytes()))
        s.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert np.all(out[0][2] == 0)


# ---- 5. the closed loop under noise, bias, periods and dropout ----------------------------------------------------------------------------------
def test_closed_loop_solves_at_the_restated_measurements(ba, start):
    traj, x0, _ = start
    cfg = _config()
    ticks, line0 = 6, 1
    s, twin = _solver(ba, start), _solver(ba, start)
    s.set_sensors(**cfg)
    ul, xl, sl = s.closed_loop(ticks, line0=line0)
    assert np.array_equal(xl[0], x0)
    r = SensorRestatement(B, **cfg)
    r.forced(0, x0)
    ys = []
    for k in range(ticks):
        ys.append(r.y.copy())                                          # what the solve of tick k knew
        r.refresh(k + 1, xl[k + 1])
    assert same(s.measured_state(), r.y) and same_stats(s.sensor_stats(), r) and r.dropped.sum() > 0
    assert np.array_equal(s.get_x0(), xl[-1])
    for k in range(ticks):                                             # the twin is GIVEN the measurement as its state
        twin.set_x0(ys[k]); twin.set_yref_from_trajectory(line0 + k, 16); twin.solve(sync=True)
        res = twin.results()
        assert np.array_equal(res["u0"], ul[k]), k
        assert np.array_equal(res["status"], sl[k]), k
    assert s.results().tobytes() == twin.results().tobytes()
    # ... and the noise is felt: the inputs differ from those of a loop that sees the true state
    plain = _solver(ba, start)
    up, _, _ = plain.closed_loop(ticks, line0=line0)
    assert np.abs(up - ul).max() > 1e-3
    for o in (s, twin, plain):
        o.close()


# ---- 6. the DOB / AMPC loop ---------------------------------------------------------------------------------------------------------------------
def test_dob_loop_equals_its_call_sequence_and_the_observer_reads_the_measurement(ba, start):
    traj, x0, _ = start
    cfg = _config()
    ticks, line0 = 5, 1
    a, ea = _solver(ba, start), _ekf(ba)
    a.set_sensors(**cfg)
    log = a.closed_loop_dob(ea, ticks=ticks, line0=line0)
    b, eb = _solver(ba, start), _ekf(ba)
    b.set_sensors(**cfg)
    seq = dict(u=[], x=[b.get_x0()], status=[], est=[])
    r = SensorRestatement(B, **cfg)
    r.forced(0, x0)
    for k in range(ticks):
        b.set_yref_from_trajectory(line0 + k, 16); b.solve()
        b.plant_step(0.05, 1)
        res = b.results()
        if k == 0:
            # one tick from a fresh EKF: a twin observer fed by hand with the restated measurement, the thrusts of the record's u0 in the
            # operation order of the observer's input kernel, and acc = (measured velocity - 0) / dt
            r.refresh(1, b.get_x0())
            y1 = r.y.copy()
            u0 = res["u0"]
            inv_rc = 1.0 / 0.026546960744430276
            t = np.stack([((-u0[:, 0] + u0[:, 1]) + u0[:, 3]) * inv_rc, ((-u0[:, 0] - u0[:, 1]) - u0[:, 3]) * inv_rc,
                          ((u0[:, 0] + u0[:, 1]) - u0[:, 3]) * inv_rc, ((u0[:, 0] - u0[:, 1]) + u0[:, 3]) * inv_rc,
                          (-u0[:, 2]) * inv_rc, (-u0[:, 2]) * inv_rc], axis=1)
            et = _ekf(ba)
            et.update(t, y1, (y1[:, 6:12] - 0.0) / 0.05)
            xt, Pt = et.state()
            et.close()
        eb.update_from_solver(b)
        if k == 0:
            assert same(b.measured_state(), y1)
            xe, Pe = eb.state()
            assert np.array_equal(xe, xt) and np.array_equal(Pe, Pt)
            assert np.abs(xe[:, :12] - b.get_x0()).max() > 1e-4        # (it is not the true state the observer saw)
        eb.apply_to_solver(b)
        seq["u"].append(res["u0"].copy()); seq["status"].append(res["status"].copy()); seq["x"].append(b.get_x0())
        seq["est"].append(eb.state()[0][:, 12:].copy())
    for key in seq:
        assert np.array_equal(log[key], np.array(seq[key])), key
    assert np.array_equal(a.get_params(), b.get_params()) and same(a.measured_state(), b.measured_state())
    sa, sb = a.sensor_stats(), b.sensor_stats()
    assert np.array_equal(sa["dropped"], sb["dropped"]) and np.array_equal(sa["err_sq"], sb["err_sq"]) and sa["refreshes"] == sb["refreshes"] == ticks
    for p, q in zip(ea.state(), eb.state()):
        assert np.array_equal(p, q)
    # the AMPC form once through
    c, ec, rc = _solver(ba, start), _ekf(ba), _rls(ba)
    c.set_sensors(**cfg)
    lg = c.closed_loop_dob(ec, rc, ba.APPLY_DISTURBANCE, ticks=ticks, line0=line0)
    assert all(np.isfinite(lg[key]).all() for key in ("u", "x", "est")) and c.sensor_stats()["refreshes"] == ticks
    for o in (a, ea, b, eb, c, ec, rc):
        o.close()


# ---- 7. refusals, and off ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_off_is_the_parent_path(ba, start):
    traj, x0, _ = start
    cfg = _config()
    s, never = _solver(ba, start), _solver(ba, start)
    with pytest.raises(RuntimeError, match="brov_sensor_last_seconds: no refresh"):
        s.sensor_last_seconds()
    with pytest.raises(RuntimeError, match="brov_sensor_measure: the sensor stage is off"):
        s.sensor_measure()
    s.set_sensors(**cfg)
    assert 0.0 < s.sensor_last_seconds() < 1.0
    y = s.measured_state()
    # refused arguments change nothing
    bad_sigma = cfg["sigma"].copy(); bad_sigma[129, 11] = np.nan
    for kw, text in ((dict(sigma=bad_sigma), "brov_sensor_set_host: sigma"), (dict(sigma=-1.0), "brov_sensor_set_host: sigma"),
                     (dict(bias=np.inf), "brov_sensor_set_host: bias"), (dict(quant=-0.5), "brov_sensor_set_host: quant"),
                     (dict(quant=np.nan), "brov_sensor_set_host: quant"), (dict(period=0), "brov_sensor_set_host: period"),
                     (dict(dropout=1.5), "brov_sensor_set_host: dropout"), (dict(dropout=np.nan), "brov_sensor_set_host: dropout")):
        with pytest.raises(RuntimeError, match=text):
            s.set_sensors(**kw)
    assert s.sensors_enabled() and np.array_equal(s.measured_state(), y)
    s.sensor_measure()                                                 # a forced refresh at the same index from the same state: the same
    assert np.array_equal(s.measured_state(), y) and s.sensor_stats()["refreshes"] == 0
    # off: a loop equals a never-on twin's (the one-launch form again), nothing is refreshed or counted, the statistics stay readable
    s.sensors_off()
    assert not s.sensors_enabled()
    la, lb = s.closed_loop(4, line0=3), never.closed_loop(4, line0=3)
    for p, q in zip(la, lb):
        assert np.array_equal(p, q)
    assert s.results().tobytes() == never.results().tobytes() and s.last_kernel_path() == never.last_kernel_path() == ba.PATH_FUSED
    assert s.sensor_stats()["refreshes"] == 0 and np.array_equal(s.measured_state(), y)
    never.close()
    s.set_sensors(**cfg)                                               # on again, at the counter's index 4
    assert same(s.measured_state(), SensorRestatement(B, **cfg).forced(4, la[1][-1]))
    # the fleet hands its candidates the vehicles' true states: refused while the stage is on, untouched after
    s.set_candidate_params("circle", np.full(B, 2.0), np.full(B, 0.5), np.zeros(B))
    f = ba.Fleet(s, 2)
    for call in (lambda: f.step(), lambda: f.closed_loop(2), lambda: f.closed_loop_dob(None, 2)):
        with pytest.raises(RuntimeError, match="sensor stage"):
            call()
    # a run that would pass index 2^24 is refused before anything is launched, under the loop's own name
    s.plant_wrench_seek(2 ** 24 - 3)
    with pytest.raises(RuntimeError, match="brov_closed_loop: the sensor stage's measurement index"):
        s.closed_loop(6)
    assert s.plant_wrench_tick() == 2 ** 24 - 3 and s.sensor_stats()["refreshes"] == 0
    s.plant_wrench_seek(2 ** 24 - 1)
    with pytest.raises(RuntimeError, match="brov_plant_step: the sensor stage's measurement index"):
        s.plant_step()
    s.plant_wrench_seek(0)
    s.sensors_off()
    assert not s.sensors_enabled()
    u, x, st, win = f.closed_loop(2)
    assert np.isfinite(x).all()
    f.step()
    f.close(); s.close()
