"""brov_eskf_update_from_solver and brov_eskf_apply_to_solver on a solver of B = 5: the inputs the hand-off synthesises (read back through
brov_eskf_get_inputs_host) and the ticks they give, against the 60-digit restatement (tests/eskf_exact.py) fed from the solver's own state.

The bar is that of tests/test_gpu_eskf_exact.py: the device's scaled error <= 4 x max(E_np, 2^-50), E_np the error of the numpy restatement
doing the same job in double (the synthesis AND the ticks, carrying its own previous velocity, position and filter state) against the same
reference -- computed here, never on the device.  The acceleration is a difference quotient: (v_I - v_I,prev) / dt loses what the subtraction
cancels, in every double implementation alike, which is what E_np measures."""
import os

import numpy as np
import pytest

import eskf_exact as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR, FLOOR = 4.0, 2.0 ** -50
B, N = 5, 20
INPUTS = ("imu", "gps_p", "gps_v", "q_meas", "thrust")


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


@pytest.fixture(scope="module")
def run(ba):
    """two ticks of solve -> plant step -> observer hand-off; everything the tests look at, read once"""
    par_vec = np.load(os.path.join(ROOT, "tests", "golden", "eskf_exact.npz"))["par"][2]      # the loop regime
    rng = np.random.default_rng(3)
    x0 = np.zeros((B, 12))
    x0[:, :3] = np.array([2.0, 0.0, -20.0]) + rng.normal(size=(B, 3)) * 0.3
    x0[:, 3:6] = rng.normal(size=(B, 3)) * np.array([0.05, 0.05, 0.4])
    x0[:, 6:12] = rng.normal(size=(B, 6)) * 0.1
    yref = np.zeros((N + 1, 16)); yref[:, :3] = [2.0, 0.0, -20.0]
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05), device=0)
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_yref(yref)
    e = ba.BatchEskf(B, X.par_apply(ba.EskfParams.default(), par_vec))
    ticks = []
    for k in range(2):
        s.solve(sync=True)
        s.plant_step(0.05)
        e.update_from_solver(s)
        ticks.append(dict(xs=s.get_x0(), u0=s.results()["u0"].copy(), inputs=e.inputs(), state=e.state(), outputs=e.outputs()))
    p_before = s.get_params()
    e.apply_to_solver(s)
    p_after = s.get_params()
    # a reset in between: the next hand-off starts afresh
    e.reset()
    e.update_from_solver(s)
    after_reset = e.inputs()
    e.close(); s.close()
    return dict(par_vec=par_vec, ticks=ticks, p_before=p_before, p_after=p_after, after_reset=after_reset)


def _reference(run):
    """per filter and tick: the reference's inputs and tick results rounded to double, and the numpy restatement's"""
    par_vec = run["par_vec"]
    p, ex = X.par_dict(par_vec), X.ExactEskf(par_vec)
    x_reset = np.zeros(X.NX); x_reset[6] = 1.0; x_reset[18] = -p["g"]
    ref, dbl = [], []
    for b in range(B):
        xm, Pm, vpm, ppm = list(x_reset), [[0.0] * X.NE for _ in range(X.NE)], None, None
        xd, Pd, vpd, ppd = x_reset.copy(), np.zeros((X.NE, X.NE)), None, None
        rb, db = [], []
        for t in run["ticks"]:
            xs, u0 = t["xs"][b], t["u0"][b]
            im, gp, gv, qm, th, vI = ex.inputs_from_state(xs, ex.thrust(u0), vpm, ppm)
            r = ex.tick(xm, Pm, im, gp, gv, qm, th)
            xm, Pm, vpm, ppm = r["x_new"], r["P_new"], vI, gp
            rr = ex.rounded(r)
            rr["inputs"] = [np.array([float(v) for v in a]) for a in (im, gp, gv, qm, th)]
            rb.append(rr)
            im, gp, gv, qm, th, vI = X.np_inputs_from_state(p, xs, X.np_thrust(u0), vpd, ppd)
            d = X.np_tick(p, xd, Pd, im, gp, gv, qm, th)
            xd, Pd, vpd, ppd = d["x_new"], d["P_new"], vI, gp
            d["inputs"] = [im, gp, gv, qm, th]
            db.append(d)
        ref.append(rb); dbl.append(db)
    return ref, dbl


def _sign(q, ref):
    return -q if np.abs(q + ref).max() < np.abs(q - ref).max() else q


def test_synthesised_inputs_and_ticks_against_the_exact_filter(run):
    ref, dbl = _reference(run)
    bad = []
    for k, t in enumerate(run["ticks"]):
        for j, name in enumerate(INPUTS):
            got = t["inputs"][j]
            e_dev = max(float(X.err_x(_sign(got[b], ref[b][k]["inputs"][j]) if name == "q_meas" else got[b], ref[b][k]["inputs"][j])) for b in range(B))
            e_np = max(float(X.err_x(dbl[b][k]["inputs"][j], ref[b][k]["inputs"][j])) for b in range(B))
            print(f"[eskf_loop] tick {k} input {name}: device {e_dev:.2e}, numpy {e_np:.2e}")
            if not e_dev <= FACTOR * max(e_np, FLOOR):
                bad.append((k, name, e_dev, e_np))
        x, P = t["state"]
        xi, xw, mp, st = t["outputs"]
        assert not st.any(), st
        for q, (name, got, key) in enumerate((("x", x, "x_new"), ("P", P, "P_new"), ("xi_world", xw, "xi_world"), ("mpc_p", mp, "mpc_p"))):
            err = X.err_state if name == "x" else (X.err_P if name == "P" else X.err_x)
            e_dev = max(float(err(got[b], ref[b][k][key])) for b in range(B))
            e_np = max(float(err(dbl[b][k][key], ref[b][k][key])) for b in range(B))
            print(f"[eskf_loop] tick {k} {name}: device {e_dev:.2e}, numpy {e_np:.2e}")
            if not e_dev <= FACTOR * max(e_np, FLOOR):
                bad.append((k, name, e_dev, e_np))
    assert not bad, bad


def test_first_call_after_reset_gives_zero_gps_velocity_and_no_acceleration_but_gravity(run):
    """the previous velocity and position are taken equal to the current ones: gps_v = 0 exactly, a_m = R'(0 - g_I)"""
    for inputs, xs in ((run["ticks"][0]["inputs"], run["ticks"][0]["xs"]), (run["after_reset"], run["ticks"][1]["xs"])):
        imu, gps_p, gps_v = inputs[0], inputs[1], inputs[2]
        assert np.array_equal(gps_v, np.zeros((B, 3)))
        assert np.array_equal(gps_p, xs[:, :3]) and np.array_equal(imu[:, 3:], xs[:, 9:12])
        for b in range(B):
            am = X.np_rot_euler(*xs[b, 3:6]).T @ np.array([0.0, 0.0, 9.81])
            assert np.abs(imu[b, :3] - am).max() < 1e-13
    assert np.abs(run["ticks"][1]["inputs"][2]).max() > 0      # the second tick has a GPS velocity


def test_apply_to_solver_writes_mpc_p_into_every_stage_and_nothing_else(run):
    mp = run["ticks"][1]["outputs"][2]
    assert np.abs(mp[:, :3]).max() > 0 and np.array_equal(mp[:, 3], np.zeros(B))
    assert np.array_equal(run["p_after"][:, :, :4], np.broadcast_to(mp[:, None, :], (B, N + 1, 4)))
    assert np.array_equal(run["p_after"][:, :, 4:], run["p_before"][:, :, 4:])
    assert not np.array_equal(run["p_after"][:, :, :3], run["p_before"][:, :, :3])
