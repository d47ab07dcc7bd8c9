"""The error-state filter at its sensors' rates on a solver of B = 5, N = 20: brov_imu_eskf_tick_from_solver behind every plant step of the IMU/GPS
stage (imu_per_tick = 3, gps_every = 2, 2 control ticks) and brov_closed_loop_eskf, the same sequence as one call.  Instance 1 drops every fix,
instance 2 (dropout 0.5, seed 2) the fixes due at 2 and 6, the others none.

The loop equals the composed sequence bit for bit.  The fix flags are those of tests/imu_restatement.py.  The filter states are held to the
60-digit filter (tests/eskf_exact.py) fed the stage's own inputs as read back from the device, at the suite's bar: a scaled error
<= 4 x max(E_np, 2^-50), E_np the worst error of the numpy filter over the same chain (every filter, every step, as that suite's chains are
held) against the same reference, computed here."""
import numpy as np
import pytest

import eskf_exact as X
from imu_restatement import ImuRestatement

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2.0 ** -50
B, N, DT, PER_TICK, EVERY, TICKS, SEED = 5, 20, 0.05, 3, 2, 2, 2
H = DT / PER_TICK
DROPOUT = np.array([0.0, 1.0, 0.5, 0.0, 0.0])
SIGMA = np.array([0.02] * 3 + [0.002] * 3 + [0.05] * 3 + [0.01] * 3)
BIAS = np.array([0.01, -0.02, 0.015, 1e-3, -2e-3, 5e-4])


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


def _par_vec():
    v = X.default_par_vector()
    v[0] = H
    v[-3], v[-2] = 1.0, 1.0      # an observer that compensates the device plant: compensate_coef = rotor_constant = 1
    return v


def _x0():
    rng = np.random.default_rng(3)
    x0 = np.zeros((B, 12))
    x0[:, :3] = np.array([2.0, 0.0, -20.0]) + rng.normal(size=(B, 3)) * 0.3
    x0[:, 3:6] = rng.normal(size=(B, 3)) * np.array([0.05, 0.05, 0.4])
    x0[:, 6:12] = rng.normal(size=(B, 6)) * 0.1
    return x0


def _pair(ba):
    """a solver with the stage on over a circle, and a filter started at the stage's first fix"""
    t = np.arange(N + TICKS + 2) * DT
    traj = np.zeros((len(t), 16))
    traj[:, 0], traj[:, 1], traj[:, 2] = 2.0 * np.cos(0.5 * t), 2.0 * np.sin(0.5 * t), -20.0
    s = ba.BatchSolver(B, ba.SolverOptions(N, DT), device=0)
    s.set_x0(_x0()); s.set_params(ba.P_NOMINAL); s.set_trajectory(traj)
    s.set_imu(H, gps_every=EVERY, seed=SEED, sigma=SIGMA, bias=BIAS, dropout=DROPOUT)
    first = s.imu()
    e = ba.BatchEskf(B, X.par_apply(ba.EskfParams.default(), _par_vec()))
    x = np.zeros((B, 22))
    x[:, :3], x[:, 6:10], x[:, 18] = first["gps_p"], first["q_meas"], -9.81
    e.set_state(x, np.broadcast_to(np.eye(21) * 0.01, (B, 21, 21)).copy())
    return s, e, x


@pytest.fixture(scope="module")
def runs(ba):
    """the sequence composed from the public calls, everything read after every filter step; then the loop as one call on a second pair"""
    s, e, x_init = _pair(ba)
    steps, logs = [], dict(u=[], x=[s.get_x0()], status=[], est=[], fix=[])
    for k in range(TICKS):
        s.set_yref_from_trajectory(k, 16)
        s.solve()
        fl = []
        for j in range(PER_TICK):
            s.plant_step(H)
            e.tick_from_solver(s)
            stage = s.imu()
            steps.append(dict(xs=s.get_x0(), stage=stage, inputs=e.inputs(), state=e.state(), outputs=e.outputs()))
            fl.append(stage["fix"])
        res = s.results()
        logs["u"].append(res["u0"].copy()); logs["status"].append(res["status"].copy()); logs["x"].append(s.get_x0())
        logs["est"].append(e.outputs()[1]); logs["fix"].append(np.array(fl))
        e.apply_to_solver(s)
    composed = dict(steps=steps, logs={k: np.array(v) for k, v in logs.items()}, x0=s.get_x0(), state=e.state(), outputs=e.outputs(),
                    p=s.get_params(), stats=s.imu_stats(), tick=s.plant_wrench_tick())
    e.close(); s.close()
    s, e, _ = _pair(ba)
    out = ba.closed_loop_eskf(s, e, TICKS, line0=0, ncols=16, dt=DT, imu_per_tick=PER_TICK)
    loop = dict(logs=out, x0=s.get_x0(), state=e.state(), outputs=e.outputs(), p=s.get_params(), stats=s.imu_stats(), tick=s.plant_wrench_tick())
    e.close(); s.close()
    return dict(composed=composed, loop=loop, x_init=x_init)


def test_the_loop_equals_the_composed_sequence_bit_for_bit(runs):
    c, l = runs["composed"], runs["loop"]
    assert c["tick"] == l["tick"] == TICKS * PER_TICK
    assert np.array_equal(c["x0"], l["x0"])
    for a, b in zip(c["state"] + c["outputs"], l["state"] + l["outputs"]):
        assert np.array_equal(a, b)
    assert np.array_equal(c["p"], l["p"]) and np.array_equal(l["p"][:, :, :4], np.broadcast_to(l["outputs"][2][:, None, :], (B, N + 1, 4)))
    assert np.abs(l["p"][:, 0, :3]).max() > 0
    for k in ("u", "x", "status", "est", "fix"):
        assert l["logs"][k].shape == c["logs"][k].shape and np.array_equal(l["logs"][k], c["logs"][k]), k
    assert not l["logs"]["wrench"].any() and not l["logs"]["status"].any()
    for k in ("samples", "fixes", "dropped", "refreshes"):
        assert np.array_equal(c["stats"][k], l["stats"][k]), k


def test_the_fix_flags_are_the_restatements(runs):
    r = ImuRestatement(B, H, gps_every=EVERY, seed=SEED, dropout=DROPOUT)
    want = np.array([r.flags_at(m) for m in range(1, TICKS * PER_TICK + 1)]).reshape(TICKS, PER_TICK, B)
    got = runs["loop"]["logs"]["fix"]
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(got.reshape(-1, B)[:, 2], [0, 0, 0, 1, 0, 0]) and not got[:, :, 1].any() and got[:, :, 0].sum() == 3
    st = runs["loop"]["stats"]
    assert np.array_equal(st["dropped"], [0, 3, 2, 0, 0]) and np.array_equal(st["fixes"], [3, 0, 1, 3, 3]) and np.array_equal(st["samples"], [6] * B)


def test_the_hand_off_reads_the_stages_sample_and_the_filter_follows_the_60_digit_filter(runs):
    steps = runs["composed"]["steps"]
    vec = _par_vec()
    ex, p = X.ExactEskf(vec), X.par_dict(vec)
    e_dev, e_np = np.zeros((B, len(steps), 4)), np.zeros((B, len(steps), 4))
    for b in range(B):
        xm, Pm = list(runs["x_init"][b]), [[0.01 if i == j else 0.0 for j in range(21)] for i in range(21)]
        xd, Pd = runs["x_init"][b].copy(), np.eye(21) * 0.01
        for n, t in enumerate(steps):
            imu, gp, gv, qm, th = (a[b] for a in t["inputs"])
            fix = bool(t["stage"]["fix"][b])
            assert np.array_equal(imu, t["stage"]["imu"][b])
            if fix:
                assert all(np.array_equal(a, t["stage"][k][b]) for a, k in ((gp, "gps_p"), (gv, "gps_v"), (qm, "q_meas")))
            r = ex.tick(xm, Pm, imu, gp, gv, qm, th, update=fix)
            xm, Pm = r["x_new"], r["P_new"]
            rr = ex.rounded(r)
            d = X.np_tick(p, xd, Pd, imu, gp, gv, qm, th, update=fix)
            xd, Pd = d["x_new"], d["P_new"]
            x, P = t["state"]
            xi, xw, mp, st = t["outputs"]
            assert st[b] == 0 and rr["status"] == 0
            for q, (name, got, key) in enumerate((("x", x[b], "x_new"), ("P", P[b], "P_new"), ("xi_world", xw[b], "xi_world"), ("mpc_p", mp[b], "mpc_p"))):
                err = X.err_state if name == "x" else (X.err_P if name == "P" else X.err_x)
                e_dev[b, n, q], e_np[b, n, q] = float(err(got, rr[key])), float(err(d[key], rr[key]))
    # as tests/test_gpu_eskf_exact.py holds its chains: per quantity, every filter at every step within FACTOR x the numpy filter's worst
    # error over the chain (all filters, all steps)
    bad = []
    for q, name in enumerate(X.QUANTITIES):
        worst_np, worst_dev = float(e_np[:, :, q].max()), float(e_dev[:, :, q].max())
        print(f"[eskf_rates] {name}: device {worst_dev:.2e}, numpy {worst_np:.2e}, ratio {worst_dev / max(worst_np, FLOOR):.2f}; "
              f"device per step " + " ".join(f"{v:.1e}" for v in e_dev[:, :, q].max(axis=0)))
        if not worst_dev <= FACTOR * max(worst_np, FLOOR):
            bad.append((name, worst_dev, worst_np))
    assert not bad, bad


def test_refusals(ba):
    s, e, _ = _pair(ba)
    e50 = ba.BatchEskf(B)                                   # the default dt = 1 / 50 is not h
    with pytest.raises(RuntimeError, match=r"brov_imu_eskf_tick_from_solver: the filter's dt is not the step h"):
        e50.tick_from_solver(s)
    with pytest.raises(RuntimeError, match=r"brov_closed_loop_eskf: the IMU stage is on and dt is not the step h"):
        ba.closed_loop_eskf(s, e, 1, dt=DT, imu_per_tick=PER_TICK + 1)
    x0 = s.get_x0()
    s.set_candidate_params("circle", np.full(B, 2.0), np.full(B, 0.5), np.zeros(B))
    f = ba.Fleet(s, B)
    for name, call in (("brov_fleet_step", lambda: f.step()), ("brov_closed_loop_fleet", lambda: f.closed_loop(2, dt_ref=DT, dt_node=DT)),
                       ("brov_closed_loop_fleet_dob", lambda: f.closed_loop_dob(None, 2, dt_ref=DT, dt_node=DT))):
        with pytest.raises(RuntimeError, match=name + r": the IMU stage of the solver's plant is on \(brov_imu_set_host\)"):
            call()
    assert np.array_equal(s.get_x0(), x0) and s.plant_wrench_tick() == 0
    f.close()
    s.imu_off()
    with pytest.raises(RuntimeError, match=r"brov_imu_eskf_tick_from_solver: the IMU stage of the solver is off"):
        e.tick_from_solver(s)
    with pytest.raises(RuntimeError, match=r"brov_closed_loop_eskf: the IMU stage of the solver is off"):
        ba.closed_loop_eskf(s, e, 1, dt=DT, imu_per_tick=PER_TICK)
    e50.close(); e.close(); s.close()
