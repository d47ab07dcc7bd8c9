"""The IMU/GPS stage of the solver's plant on the device (brov_imu_*), B = 5: the stage alone against the 60-digit inputs of
tests/eskf_exact.py, its noise and bias bit for bit against numpy, and the stage behind plant steps -- flags, held values, both gps_v divisors,
restarts, statistics, refusals -- against tests/imu_restatement.py.

Bars.  Noiseless values against the 60-digit ones, q_meas against the restatement: a scaled error <= 4 x max(E_np, 2^-50), the suite's own
(tests/test_gpu_eskf_exact.py), E_np the error of eskf_exact.np_inputs_from_state against the same 60-digit values, computed here.  Flags,
statistics, and (noiseless + bias) + sigma * n: bit for bit."""
import numpy as np
import pytest

import eskf_exact as X
from imu_restatement import ImuRestatement, channel_noise

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2.0 ** -50
B, N, H = 5, 20, 0.01


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


def _x0(seed=3):
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 12))
    x0[:, :3] = np.array([2.0, 0.0, -20.0]) + rng.normal(size=(B, 3)) * 0.3
    x0[:, 3:6] = rng.normal(size=(B, 3)) * np.array([0.05, 0.05, 0.4])
    x0[:, 6:12] = rng.normal(size=(B, 6)) * 0.1
    return x0


@pytest.fixture(scope="module")
def solver(ba):
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05), device=0)
    yref = np.zeros((N + 1, 16)); yref[:, :3] = [2.0, 0.0, -20.0]
    s.set_x0(_x0()); s.set_params(ba.P_NOMINAL); s.set_yref(yref)
    s.solve(sync=True)          # a record for the plant steps
    yield s
    s.close()


def _par(h):
    v = X.default_par_vector()
    v[0] = v[1] = h
    return v


def _f(v):
    return np.array([float(t) for t in v])


def test_the_stage_alone_against_the_60_digit_inputs_and_its_noise_bit_for_bit(ba, solver):
    s = solver
    s.imu_off()
    rng = np.random.default_rng(8)
    x = _x0(4); v_prev = rng.normal(size=(B, 3)) * 0.1; p_last = x[:, :3] - rng.normal(size=(B, 3)) * 0.01
    m, every = 6, 2      # (a power of two: the velocity times gps_every below is exact)
    m_last = np.full(B, m - every, dtype=np.int32)
    s.set_imu(H, gps_every=every, seed=5)
    clean = s.imu_eval(m, x, v_prev, p_last, m_last)
    assert np.array_equal(clean["fix"], np.ones(B))
    ex, p = X.ExactEskf(_par(H)), X.par_dict(_par(H))
    worst, e_np = 0.0, 0.0
    for b in range(B):
        imu, gp, gv, qm, _, _ = ex.inputs_from_state(x[b], np.zeros(6), v_prev[b], p_last[b])
        n_imu, _, n_gv, n_qm, _, _ = X.np_inputs_from_state(p, x[b], np.zeros(6), v_prev[b], p_last[b])
        worst = max(worst, X.err_x(clean["imu"][b], _f(imu)), X.err_x(clean["gps_v"][b] * every, _f(gv)), X.err_x(clean["q_meas"][b], _f(qm)))
        e_np = max(e_np, X.err_x(n_imu, _f(imu)), X.err_x(n_gv, _f(gv)), X.err_x(n_qm, _f(qm)))
        assert np.array_equal(clean["gps_p"][b], x[b, :3])
    print(f"[imu] stage alone against 60 digits: device {worst:.2e}, numpy {e_np:.2e}")
    assert worst <= FACTOR * max(e_np, FLOOR)
    # noise and bias: (noiseless + bias) + sigma * n, bit for bit; q_meas within the bar of the restatement
    sigma = rng.uniform(0.001, 0.05, (B, 12)); bias = rng.normal(size=(B, 6)) * 0.01
    s.set_imu(H, gps_every=every, seed=5, sigma=sigma, bias=bias)
    noisy = s.imu_eval(m, x, v_prev, p_last, m_last)
    n = {slot: channel_noise(5, B, m, slot, 3) for slot in (16, 19, 22, 25)}
    assert np.array_equal(noisy["imu"][:, :3], (clean["imu"][:, :3] + bias[:, :3]) + sigma[:, :3] * n[16])
    assert np.array_equal(noisy["imu"][:, 3:], (clean["imu"][:, 3:] + bias[:, 3:]) + sigma[:, 3:6] * n[19])
    assert np.array_equal(noisy["gps_p"], x[:, :3] + sigma[:, 6:9] * n[22])
    assert np.array_equal(noisy["gps_v"], (noisy["gps_p"] - p_last) / (float(every) * H))
    r = ImuRestatement(B, H, gps_every=every, seed=5, sigma=sigma, bias=bias)
    want = r.sample(m, x, v_prev, p_last, m_last)
    eq = max(float(X.err_x(X.np_unit(noisy["q_meas"][b]), want["q_meas"][b])) for b in range(B))
    print(f"[imu] q_meas against the restatement: {eq:.2e}")
    assert eq <= FACTOR * max(e_np, FLOOR) and np.abs(noisy["q_meas"] - clean["q_meas"]).max() > 1e-4
    # an index at which no fix is due: flags 0, the GPS values come back as zeros; the other divisor; no earlier fix
    off = s.imu_eval(m + 1, x, v_prev, p_last, m_last)
    assert not off["fix"].any() and not off["gps_p"].any() and not off["q_meas"].any()
    s.set_imu(H, gps_every=every, seed=5, sigma=sigma, bias=bias, flags=ba.IMU_GPSV_ELAPSED)
    m_last2 = np.array([0, 4, 4, 0, 4], dtype=np.int32)
    el = s.imu_eval(m, x, v_prev, p_last, m_last2)
    assert np.array_equal(el["gps_v"], (noisy["gps_p"] - p_last) / ((m - m_last2)[:, None].astype(float) * H))
    none = s.imu_eval(m, x, v_prev, p_last, np.full(B, -1, dtype=np.int32))
    assert not none["gps_v"].any() and np.array_equal(none["gps_p"], noisy["gps_p"])
    s.imu_off()


def test_the_stage_behind_plant_steps(ba, solver):
    """6 plant steps, gps_every = 2, seed 2: instance 1 drops every fix, instance 2 (dropout 0.5) the fixes at 2 and 6.  Flags and statistics
    are the restatement's; values are held between fixes; gps_v divides by the nominal period (after the dropped fix at 2 instance 2 has the
    velocity of four steps over two); a plant step with dt != h is refused; restart and set_x0 take a fix with gps_v = 0."""
    s = solver
    x0 = _x0()
    s.plant_wrench_seek(0); s.set_x0(x0)
    sigma = np.zeros((B, 12)); sigma[:, 6:9] = 0.01
    drop = np.array([0.0, 1.0, 0.5, 0.0, 0.0])
    s.set_imu(H, gps_every=2, seed=2, sigma=sigma, dropout=drop)
    r = ImuRestatement(B, H, gps_every=2, seed=2, sigma=sigma, dropout=drop)
    r.restart(0, x0)
    o = s.imu()
    assert np.array_equal(o["fix"], np.ones(B)) and not o["gps_v"].any() and np.array_equal(o["gps_p"], r.gps_p)
    assert not any(v.any() for k, v in s.imu_stats().items() if k != "refreshes")
    with pytest.raises(RuntimeError, match=r"brov_plant_step: the IMU stage is on and dt is not the step h"):
        s.plant_step(0.05)
    assert s.plant_wrench_tick() == 0 and np.array_equal(s.get_x0(), x0)
    flags, prev = [], o
    for m in range(1, 7):
        s.plant_step(H)
        x = s.get_x0()
        want = r.refresh(m, x)
        o = s.imu()
        flags.append(o["fix"].copy())
        assert np.array_equal(o["fix"], want), (m, o["fix"], want)
        f = o["fix"].astype(bool)
        for k in ("gps_p", "gps_v", "q_meas"):
            assert np.array_equal(o[k][~f], prev[k][~f]), (m, k)                 # held
        assert np.array_equal(o["gps_p"][f], r.gps_p[f]) and np.array_equal(o["imu"][:, 3:], x[:, 9:12])
        assert np.array_equal(o["gps_v"][f], r.gps_v[f]), m
        prev = o
    flags = np.array(flags)
    assert np.array_equal(flags[:, 2], [0, 0, 0, 1, 0, 0]) and not flags[:, 1].any() and np.array_equal(flags[:, 0], [0, 1, 0, 1, 0, 1])
    st = s.imu_stats()
    assert np.array_equal(st["samples"], r.samples) and np.array_equal(st["fixes"], r.fixes) and np.array_equal(st["dropped"], r.dropped)
    assert st["refreshes"] == 6 and np.array_equal(st["dropped"], [0, 3, 2, 0, 0]) and s.imu_last_seconds() > 0
    # restart: a fix for everyone, the dropper included, gps_v = 0, gravity alone; the statistics stay
    s.imu_restart()
    o = s.imu()
    x = s.get_x0()
    assert np.array_equal(o["fix"], np.ones(B)) and not o["gps_v"].any()
    for b in range(B):
        assert np.abs(o["imu"][b, :3] - X.np_rot_euler(*x[b, 3:6]).T @ np.array([0.0, 0.0, 9.81])).max() < 1e-12
    assert np.array_equal(s.imu_stats()["samples"], r.samples)
    # set_x0 while the stage is on restarts it too
    s.set_x0(x0)
    r.restart(6, x0)
    o = s.imu()
    assert np.array_equal(o["fix"], np.ones(B)) and not o["gps_v"].any() and np.array_equal(o["gps_p"], r.gps_p)
    assert np.array_equal(s.imu_stats()["samples"], r.samples)
    s.imu_off()
    s.plant_step(0.05)                                  # off: any dt again
    s.plant_wrench_seek(0); s.set_x0(x0)


def test_the_plant_does_not_see_the_stage(ba, solver):
    """the same plant steps with the stage on and off: the states bit for bit"""
    s = solver
    x0 = _x0(9)
    runs = []
    for on in (False, True):
        s.plant_wrench_seek(0); s.set_x0(x0)
        if on:
            s.set_imu(H, gps_every=2, seed=1, sigma=0.01, bias=0.001, dropout=0.3)
        xs = []
        for _ in range(4):
            s.plant_step(H)
            xs.append(s.get_x0())
        runs.append(np.array(xs))
        s.imu_off()
    assert np.array_equal(runs[0], runs[1]) and not np.array_equal(runs[0][0], runs[0][3])
    s.plant_wrench_seek(0); s.set_x0(_x0())
