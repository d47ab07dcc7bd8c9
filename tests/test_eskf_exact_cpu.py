"""The yardstick of the error-state filter without a GPU: the numpy restatement of tests/eskf_exact.py against the fixture (the stored E_np is
reproduced), and known answers that depend on neither restatement."""
import os

import numpy as np
import pytest

import eskf_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    g = np.load(os.path.join(ROOT, "tests", "golden", "eskf_exact.npz"))
    d = {k: g[k] for k in g.files}
    d["family_names"] = list(d["families"])
    return d


def _case(fx, k):
    return (fx["x0"][k], X.from_triu(fx["P0u"][fx["input"][k]]), fx["imu"][k], fx["gps_p"][k], fx["gps_v"][k], fx["qm"][k], fx["thrust"][k])


def test_fixture_is_small_and_complete(fx):
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "eskf_exact.npz"))
    assert size <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "ekf_exact.npz")) and size < 2 ** 20
    assert tuple(fx["regimes"]) == ("shipped", "varied", "loop") and tuple(fx["quantities"]) == X.QUANTITIES
    assert np.array_equal(fx["par"][0], X.default_par_vector())
    q, r = X.par_dict(fx["par"][1])["Q"], X.par_dict(fx["par"][1])["R12"]
    assert len(set(q)) == 21 and len(set(r)) == 12                       # pairwise different: a wrong index cannot hide
    assert np.isfinite(fx["E_np"]).all()
    for ri in range(3):
        for fi in range(len(fx["family_names"]) - 1):
            assert ((fx["regime"] == ri) & (fx["family"] == fi)).sum() >= 2, (ri, fi)


def test_numpy_restatement_reproduces_the_stored_error(fx):
    """every single tick and every chain in plain double against the stored 60-digit results: the worst error per regime, family and quantity
    is the fixture's E_np, and the statuses are the reference's"""
    po = fx["family_names"].index("predict_only")
    E = np.zeros_like(fx["E_np"])
    for k in range(len(fx["regime"])):
        ri, fi = int(fx["regime"][k]), int(fx["family"][k])
        d = X.np_tick(X.par_dict(fx["par"][ri]), *_case(fx, k), update=fi != po)
        assert d["status"] == fx["status"][k]
        e = X.errors((d["x_new"][None], d["P_new"][None], d["xi_world"][None], d["mpc_p"][None]),
                     (fx["xn"][k][None], X.from_triu(fx["Pnu"][k])[None], fx["xw"][k][None], fx["mp"][k][None]))[:, 0]
        E[ri, fi] = np.maximum(E[ri, fi], e)
    ci = fx["family_names"].index("chain")
    for ri in range(3):
        p = X.par_dict(fx["par"][ri])
        K, B = fx["chain_xn"].shape[1:3]
        for b in range(B):
            x, P = fx["chain_x0"][ri, b], X.from_triu(fx["P0u"][fx["chain_input"][ri, b]])
            for k in range(K):
                d = X.np_tick(p, x, P, *(fx["chain_" + n][ri, k, b] for n in ("imu", "gps_p", "gps_v", "qm", "thrust")), update=bool(fx["chain_update"][ri, k]))
                x, P = d["x_new"], d["P_new"]
                e = X.errors((x[None], P[None], d["xi_world"][None], d["mpc_p"][None]),
                             (fx["chain_xn"][ri, k, b][None], X.from_triu(fx["chain_Pnu"][ri, k, b])[None], fx["chain_xw"][ri, k, b][None],
                              fx["chain_mp"][ri, k, b][None]))[:, 0]
                E[ri, ci] = np.maximum(E[ri, ci], e)
    assert np.allclose(E, fx["E_np"], rtol=1e-9, atol=0), np.abs(E - fx["E_np"]).max()
    assert E.max() < 1e-11                                                # the families are well conditioned


def test_exact_filter_agrees_with_the_fixture_on_one_case_and_chains_at_60_digits(fx):
    mp = pytest.importorskip("mpmath")
    assert mp is not None
    k = int(np.nonzero((fx["regime"] == 1) & (fx["family"] == 0))[0][0])
    ex = X.ExactEskf(fx["par"][1])
    r = ex.tick(*_case(fx, k))
    rr = ex.rounded(r)
    assert np.array_equal(rr["x_new"], fx["xn"][k]) and np.array_equal(X.to_triu(rr["P_new"]), fx["Pnu"][k])
    assert rr["status"] == 0 and (rr["pivots"] > 0).all() and np.array_equal(rr["pivots"], fx["pivots"][k])
    # P is symmetric to the working precision, and a second tick takes the state as mpf
    asym = max(abs(r["P_new"][i][j] - r["P_new"][j][i]) for i in range(X.NE) for j in range(i))
    assert asym < mp.mpf(10) ** -50
    r2 = ex.tick(r["x_new"], r["P_new"], fx["imu"][k], update=False)
    assert type(r2["x_new"][0]) is type(r["x_new"][0]) and r2["status"] == 0


# ---- known answers, independent of both restatements ---------------------------------------------------------------------------------------------
def _random_case(seed):
    rng = np.random.default_rng(seed)
    x = np.zeros(X.NX)
    x[0:6] = rng.normal(size=6)
    x[6:10] = X.np_unit(rng.normal(size=4))
    x[10:16] = rng.normal(size=6) * 0.01
    x[16:19] = [0, 0, -9.81]
    x[19:22] = rng.normal(size=3)
    A = rng.normal(size=(X.NE, X.NE)) * 0.2
    return rng, x, A @ A.T + np.eye(X.NE) * 0.05


def test_with_zero_covariance_the_update_changes_nothing_but_P():
    p = X.par_dict(X.default_par_vector())
    rng, x, _ = _random_case(1)
    p["Q"] = np.zeros(21)
    d = X.np_tick(p, x, np.zeros((X.NE, X.NE)), rng.normal(size=6), rng.normal(size=3), rng.normal(size=3), X.np_unit(rng.normal(size=4)), rng.normal(size=6))
    assert d["status"] == 0 and np.array_equal(d["x_new"], d["x_pred"]) and np.array_equal(d["P_new"], np.zeros((X.NE, X.NE)))
    p["Q"] = np.full(21, 0.001)      # P_pred = diag(Q): the gain is not zero, the state moves, and P is Q - Q H' (H Q H' + R)^-1 H Q, a diagonal
    d = X.np_tick(p, x, np.zeros((X.NE, X.NE)), rng.normal(size=6), rng.normal(size=3), rng.normal(size=3), X.np_unit(rng.normal(size=4)), rng.normal(size=6))
    want = np.full(21, 0.001)
    want[list(X.HSEL)] = 0.001 - 0.001 ** 2 / (0.001 + p["R12"])
    assert np.allclose(d["P_new"], np.diag(want), rtol=1e-13, atol=1e-20) and not np.array_equal(d["x_new"][0:3], d["x_pred"][0:3])


def test_with_zero_noise_and_zero_imu_the_predict_keeps_v_and_q_and_P_is_a_hand_written_F_P_Ft():
    p = X.par_dict(X.default_par_vector())
    p["Q"] = np.zeros(21)
    rng, x, P = _random_case(2)
    x[10:19] = 0.0                                  # no biases, no gravity: a = w = 0
    d = X.np_tick(p, x, P, np.zeros(6), update=False)
    assert np.array_equal(d["x_pred"][3:6], x[3:6]) and np.allclose(d["x_pred"][6:10], x[6:10], rtol=0, atol=2e-16)
    assert np.allclose(d["x_pred"][0:3], x[0:3] + x[3:6] * p["dt"], rtol=0, atol=1e-15)
    dt, R = p["dt"], X.np_rot(x[6:10])
    F = np.eye(21)                                  # written out entry by entry
    for r in range(3):
        F[r, 3 + r] = dt
        F[3 + r, 15 + r] = dt
        F[6 + r, 9 + r] = -dt
        for c in range(3):
            F[3 + r, 12 + c] = -R[r, c] * dt        # -R hat(0) dt = 0; exp(0) = I
    assert np.allclose(d["P_pred"], F @ P @ F.T, rtol=1e-13, atol=1e-15)


def test_dense_H_and_F_give_what_the_structured_path_gives():
    p = X.par_dict(np.load(os.path.join(ROOT, "tests", "golden", "eskf_exact.npz"))["par"][1])
    rng, x, P = _random_case(3)
    args = (rng.normal(size=6), rng.normal(size=3), rng.normal(size=3), X.np_unit(rng.normal(size=4)), rng.normal(size=6))
    a, w = args[0][0:3] - x[13:16], args[0][3:6] - x[10:13]
    Rn = X.np_rot(X.np_tick(p, x, P, args[0], update=False)["x_pred"][6:10])
    Pd, Ps = X.np_predict_cov(p, P, Rn, a, w, structured=False), X.np_predict_cov(p, P, Rn, a, w, structured=True)
    assert np.abs(Pd - Ps).max() <= 1e-14 * np.abs(Pd).max()
    (Sd, PHd), (Ss, PHs) = X.np_S(p, Pd, structured=False), X.np_S(p, Pd, structured=True)
    assert np.array_equal(Sd, Ss) and np.array_equal(PHd, PHs)          # a selection: the dense products add zeros
    d, s = X.np_tick(p, x, P, *args, structured=False), X.np_tick(p, x, P, *args, structured=True)
    assert np.abs(d["P_new"] - s["P_new"]).max() <= 1e-13 * np.abs(d["P_new"]).max() and np.abs(d["x_new"] - s["x_new"]).max() < 1e-12
    H = X.np_H()
    assert H.shape == (12, 21) and np.abs(H).sum() == 12 and H[9, 18] == -1 and H[11, 20] == -1 and H[8, 8] == 1 and H[:, 9:18].any() == False  # noqa: E712


def test_R_xi_is_xi_world(fx):
    for k in (0, 25, 50):
        q, xi = fx["xn"][k][6:10], fx["xn"][k][19:22]
        w, x, y, z = q
        v = np.array([x, y, z])
        rot = xi + 2 * w * np.cross(v, xi) + 2 * np.cross(v, np.cross(v, xi))      # Rodrigues' form for a unit quaternion, not R(q)
        assert np.abs(rot - fx["xw"][k]).max() < 1e-13 * max(1.0, np.abs(xi).max())
        assert np.array_equal(fx["xi"][k], xi)
