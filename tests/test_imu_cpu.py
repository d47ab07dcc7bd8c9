"""The IMU/GPS stage's numpy restatement (tests/imu_restatement.py) without a GPU: against the 60-digit inputs of tests/eskf_exact.py, the
multi-rate filter chain it drives against the 60-digit filter, its noise counters against the sensor stage's, and the dropout pattern the GPU
tests use.

The bar is the suite's own (tests/test_gpu_eskf_exact.py): a scaled error <= 4 x max(E_np, 2^-50).  For the filter E_np is the fixture's, of the
`chain` family of the `loop` regime; for the inputs, which the fixture does not hold, it is the error of eskf_exact.np_inputs_from_state -- the
suite's existing numpy statement of the same geometry -- against the same 60-digit values, computed here."""
import os

import numpy as np

import eskf_exact as X
import sensor_restatement as SR
from imu_restatement import ImuRestatement, channel_noise, dropout_draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR, FLOOR = 4.0, 2.0 ** -50
H = 0.01


def _states(B, K, seed=3):
    """K + 1 smooth 12-states of B instances, h apart: positions, Euler angles, body velocities and rates of a manoeuvring vehicle"""
    rng = np.random.default_rng(seed)
    x0 = np.concatenate([rng.uniform(-3, 3, (B, 2)), rng.uniform(-20, -5, (B, 1)), rng.uniform(-0.4, 0.4, (B, 2)), rng.uniform(-3, 3, (B, 1)),
                         rng.uniform(-0.8, 0.8, (B, 3)), rng.uniform(-0.3, 0.3, (B, 3))], axis=1)
    rate = np.concatenate([rng.uniform(-0.8, 0.8, (B, 3)), rng.uniform(-0.3, 0.3, (B, 3)), rng.uniform(-1, 1, (B, 3)), rng.uniform(-0.5, 0.5, (B, 3))], axis=1)
    return np.array([x0 + k * H * rate + 0.5 * (k * H) ** 2 * rate[:, ::-1] for k in range(K + 1)])


def _par(h):
    v = X.default_par_vector()
    v[0] = v[1] = h      # dt = gps_dt = h
    v[-3], v[-2] = 1.0, 1.0
    return v


def _f(v):
    return np.array([float(t) for t in v])


def test_noiseless_chain_gives_the_60_digit_inputs():
    """6 plant steps, gps_every = 2, sigma = bias = 0: IMU sample, position, attitude of every step and the fix's velocity against
    ExactEskf.inputs_from_state called per step with dt = gps_dt = h.  The exact call differences the position over ONE period h from the
    previous value it is given -- here the last fix, two steps back --, the stage over the nominal gps_every * h: its velocity times gps_every
    (a power of two: exact) is compared."""
    B, K, every = 2, 6, 2
    xs = _states(B, K)
    ex, p = X.ExactEskf(_par(H)), X.par_dict(_par(H))
    r = ImuRestatement(B, H, gps_every=every)
    r.restart(0, xs[0])
    assert np.array_equal(r.fix, [1, 1]) and not r.gps_v.any()
    assert np.abs(r.imu[:, :3] - X.np_rot_euler(*xs[0][0, 3:6]).T[None] @ np.array([0, 0, 9.81]))[0].max() < 1e-12      # gravity alone
    v_ex = [ex.inputs_from_state(xs[0][b], np.zeros(6))[5] for b in range(B)]
    v_np = [X.np_inputs_from_state(p, xs[0][b], np.zeros(6))[5] for b in range(B)]
    p_last = xs[0][:, :3].copy()
    worst, e_np = 0.0, 0.0
    for m in range(1, K + 1):
        fix = r.refresh(m, xs[m])
        assert np.array_equal(fix, [int(m % every == 0)] * B)
        for b in range(B):
            imu, gp, gv, qm, _, vI = ex.inputs_from_state(xs[m][b], np.zeros(6), v_ex[b], p_last[b])
            n_imu, n_gp, n_gv, n_qm, _, n_vI = X.np_inputs_from_state(p, xs[m][b], np.zeros(6), v_np[b], p_last[b])
            v_ex[b], v_np[b] = vI, n_vI
            worst = max(worst, X.err_x(r.imu[b], _f(imu)))
            e_np = max(e_np, X.err_x(n_imu, _f(imu)))
            if fix[b]:
                worst = max(worst, X.err_x(r.gps_p[b], _f(gp)), X.err_x(r.gps_v[b] * every, _f(gv)), X.err_x(r.q_meas[b], _f(qm)))
                e_np = max(e_np, X.err_x(n_gv, _f(gv)), X.err_x(n_qm, _f(qm)))
        p_last[fix.astype(bool)] = xs[m][fix.astype(bool), :3]
        held = ~fix.astype(bool)
        if m == 1:
            assert held.all() and np.array_equal(r.gps_p, xs[0][:, :3]) and not r.gps_v.any()      # held from the restart
    bar = FACTOR * max(e_np, FLOOR)
    print(f"inputs: restatement {worst:.2e}, np_inputs_from_state {e_np:.2e}, bar {bar:.2e}")
    assert worst <= bar
    assert np.array_equal(r.samples, [K] * B) and np.array_equal(r.fixes, [K // every] * B) and not r.dropped.any()


def test_multi_rate_chain_of_the_numpy_filter_stays_within_the_bar_of_the_60_digit_filter():
    """predict-only and update ticks alternating as the stage's flags say (gps_every = 2, 6 steps, noise and bias on), the numpy filter and the
    60-digit filter each carrying their own state, both fed the stage's own inputs"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "eskf_exact.npz"))
    ri, fi = list(g["regimes"]).index("loop"), list(g["families"]).index("chain")
    e_np = g["E_np"][ri, fi]
    B, K, every = 2, 6, 2
    xs = _states(B, K, seed=5)
    sigma = np.array([0.02] * 3 + [0.002] * 3 + [0.05] * 3 + [0.01] * 3)
    r = ImuRestatement(B, H, gps_every=every, seed=11, sigma=sigma, bias=[0.01, -0.02, 0.015, 1e-3, -2e-3, 5e-4])
    vec = _par(H)
    ex, p = X.ExactEskf(vec), X.par_dict(vec)
    r.restart(0, xs[0])
    thrust = np.array([1.0, -0.5, 0.25, 0.75, -2.0, -2.0])
    x_np = [np.concatenate([xs[0][b, :3], r.v_prev[b], r.q_meas[b], np.zeros(6), [0, 0, -9.81], np.zeros(3)]) for b in range(B)]
    P_np = [np.eye(21) * 0.01 for _ in range(B)]
    x_ex, P_ex = [x.copy() for x in x_np], [P.copy() for P in P_np]
    errs, updates = [], 0
    for m in range(1, K + 1):
        fix = r.refresh(m, xs[m])
        for b in range(B):
            args = (r.imu[b], r.gps_p[b], r.gps_v[b], r.q_meas[b], thrust)
            o_np = X.np_tick(p, x_np[b], P_np[b], *args, update=bool(fix[b]))
            o_ex = ex.tick(x_ex[b], P_ex[b], *args, update=bool(fix[b]))
            assert o_np["status"] == 0 and o_ex["status"] == 0
            x_np[b], P_np[b] = o_np["x_new"], o_np["P_new"]
            x_ex[b], P_ex[b] = o_ex["x_new"], o_ex["P_new"]
            rd = ex.rounded(o_ex)
            errs.append(X.errors((o_np["x_new"][None], o_np["P_new"][None], o_np["xi_world"][None], o_np["mpc_p"][None]),
                                 (rd["x_new"][None], rd["P_new"][None], rd["xi_world"][None], rd["mpc_p"][None]))[:, 0])
            updates += int(fix[b])
    worst = np.max(errs, axis=0)
    print("multi-rate chain:", " ".join(f"{q} {w:.2e} (E_np {e:.2e})" for q, w, e in zip(X.QUANTITIES, worst, e_np)))
    assert updates == B * (K // every)
    for q in range(4):
        assert worst[q] <= FACTOR * max(float(e_np[q]), FLOOR), (X.QUANTITIES[q], worst[q], e_np[q])


def test_noise_channels_are_disjoint_from_the_sensor_stages():
    """same seed, same instance and index: the stage's slots 16..28 are none of the sensor stage's 0..12, its keys are other keys and its
    variates other variates"""
    seed, B, m = 7, 64, 9
    sensor = SR.noise(seed, np.arange(B)[:, None], m, np.arange(12)[None, :])
    imu = np.concatenate([channel_noise(seed, B, m, s, 3) for s in (16, 19, 22, 25)], axis=1)
    assert imu.shape == sensor.shape == (B, 12)
    assert not np.any(imu == sensor) or np.mean(imu == sensor) < 0.01
    assert abs(np.corrcoef(imu.ravel(), sensor.ravel())[0, 1]) < 5 / np.sqrt(imu.size)
    keys = lambda c: set(int(k) for j in range(3) for k in SR.hashes(seed, np.arange(B)[:, None], m, np.asarray(c)[None, :], j).ravel())
    assert not keys(range(0, 13)) & keys(range(16, 29))
    assert not np.array_equal(dropout_draw(seed, np.arange(B), m), SR.dropout_draw(seed, np.arange(B), m))


def test_the_dropout_pattern_the_gpu_tests_use():
    """seed 2, instance 2, dropout 0.5, gps_every 2: the fixes due at 2, 4, 6 are dropped, kept, dropped"""
    u = dropout_draw(2, 2, np.array([2, 4, 6]))
    assert np.allclose(u, [0.325, 0.511, 0.205], atol=5e-4), u
    r = ImuRestatement(5, H, gps_every=2, seed=2, dropout=[0, 1, 0.5, 0, 0])
    flags = np.array([r.flags_at(m) for m in range(1, 7)])
    assert np.array_equal(flags[:, 2], [0, 0, 0, 1, 0, 0]) and not flags[:, 1].any()
    assert np.array_equal(flags[:, 0], [0, 1, 0, 1, 0, 1]) and np.array_equal(flags[:, 0], flags[:, 3])
