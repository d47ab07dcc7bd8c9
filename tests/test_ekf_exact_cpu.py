"""The 60-digit filter (tests/ekf_exact.py) and its fixture (tests/golden/ekf_exact.npz, scripts/make_ekf_exact_golden.py), checked without a
GPU: the fixture against a recomputation, the conditions its cases are meant to meet on the reference alone, and the teeth of the bar the
GPU test holds the kernel to (tests/test_gpu_ekf_exact.py): eight deliberate mistakes in the numpy restatement, each of which must exceed it
a hundredfold in the tight regime -- with a report of which of them the 1e-6 / 1e-5 tolerances of tests/test_gpu_ekf.py let through."""
import os
import sys

import numpy as np
import pytest

import test_oracle_ekf as T
from ekf_exact import QUANTITIES, Doubles, ExactEkf, errors, from_triu, par_dict, to_triu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import make_ekf_exact_golden as G  # noqa: E402

FACTOR, FLOOR = 4.0, 2.0 ** -50          # the bar of tests/test_gpu_ekf_exact.py
TRIG_DOMAIN = 1e6                        # rad: sincos_pio2's specified range (bluerov2_model.hpp)


@pytest.fixture(scope="module")
def fx():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ekf_exact.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def doubles(fx):
    return [Doubles(v) for v in fx["par"]]


def _case(fx, c):
    m = fx["input"][c]
    return fx["x0"][m], from_triu(fx["P0u"][m]), fx["thrust"][c], fx["y12"][c], fx["acc"][c]


def _ref(fx, c):
    return fx["xn"][c], from_triu(fx["Pnu"][c]), fx["wf"][c], fx["mp"][c]


def test_names_and_parameters_are_the_generators(fx):
    assert tuple(fx["regimes"]) == G.REGIMES and tuple(fx["families"]) == G.FAMILIES and tuple(fx["quantities"]) == QUANTITIES
    from ekf_exact import par_vector
    from oracle.oracle_ffi import EkfOracle
    par = G.regime_params(par_vector(EkfOracle().par))
    for ri, r in enumerate(G.REGIMES):
        assert np.array_equal(fx["par"][ri], par[r]), r
    p = {r: par_dict(fx["par"][ri]) for ri, r in enumerate(G.REGIMES)}
    assert p["shipped"]["fd_step"] == 1e-6 and p["shipped"]["R"] == 0.05 ** 4 / 4
    assert (p["tight"]["fd_step"], p["tight"]["R"]) == (2.0 ** -7, 1.0) and (p["mid"]["fd_step"], p["mid"]["R"]) == (2.0 ** -10, 1e-2)
    for r in G.REGIMES[1:]:       # 18 pairwise different entries over the default's range
        q = p[r]["Q"]
        assert len(set(q)) == 18 and q.min() == p["shipped"]["Q"].min() and np.isclose(q.max(), p["shipped"]["Q"].max(), rtol=1e-15), r
    assert len(set(p["shipped"]["Q"])) == 2
    d = p["device_loop"]
    assert not d["K"][12:24].any() and d["K"][:12].any() and d["compensate_coef"] == 1.0 and d["rotor_constant"] == 1.0 and d["fd_step"] == 2.0 ** -7
    v = p["varied"]
    for f in ("dt", "mass"):
        assert v[f] != p["tight"][f]
    for f in ("added_mass", "Dl", "Dnl"):
        assert (v[f] != p["tight"][f]).sum() >= 4, f


def test_fixture_is_what_the_exact_filter_gives_bit_for_bit(fx):
    """the first case of every regime and family, and the first filter of both chains, recomputed with mpmath"""
    for ri in range(len(G.REGIMES)):
        X = ExactEkf(fx["par"][ri])
        for fi in range(len(G.SINGLE)):
            c = int(np.nonzero((fx["regime"] == ri) & (fx["family"] == fi))[0][0])
            r = X.tick_double(*_case(fx, c))
            assert r["status"] == fx["status"][c]
            assert np.array_equal(r["x_new"], fx["xn"][c]) and np.array_equal(to_triu(r["P_new"]), fx["Pnu"][c]), (ri, fi)
            assert np.array_equal(r["P_new"], r["P_new"].T)
            assert np.array_equal(r["wf"], fx["wf"][c]) and np.array_equal(r["mpc_p"], fx["mp"][c]), (ri, fi)
            assert r["pivots"][0] == fx["piv_first"][c] and np.nanmin(r["pivots"]) == fx["piv_min"][c]
            k = np.nonzero(fx["pred_case"] == c)[0]
            if len(k):
                assert np.array_equal(r["x_pred"], fx["pred_x"][k[0]]) and np.array_equal(to_triu(r["P_pred"]), fx["pred_Pu"][k[0]])
            if r["status"] == 1:
                assert np.array_equal(r["x_new"], r["x_pred"]) and np.array_equal(r["P_new"], r["P_pred"])
    assert len(fx["pred_case"]) == len(G.REGIMES)
    for ci, ri in enumerate(fx["chain_regime"]):
        X = ExactEkf(fx["par"][ri])
        x, P = fx["chain_x0"][0], from_triu(fx["chain_P0u"][0])
        for k in range(G.CHAIN_TICKS):
            out = X.tick(x, P, fx["chain_thrust"][ci, k, 0], fx["chain_y12"][ci, k, 0], fx["chain_acc"][ci, k, 0])
            x, P = out["x_new"], out["P_new"]         # carried at 60 digits
            r = X.rounded(out)
            assert np.array_equal(r["x_new"], fx["chain_xn"][ci, k, 0]) and np.array_equal(to_triu(r["P_new"]), fx["chain_Pnu"][ci, k, 0]), (ci, k)
            assert np.array_equal(r["wf"], fx["chain_wf"][ci, k, 0]) and np.array_equal(r["mpc_p"], fx["chain_mp"][ci, k, 0])


def test_stored_errors_of_the_two_double_implementations_recompute(fx, doubles):
    """E_orc and E_np from the oracle and the restatement, every case and every chained tick.  With the same compiler, libm and BLAS they are
    the stored numbers; another machine's may sum in another order, and a correct double evaluation is then within the bar's own factor."""
    nr, nf = len(G.REGIMES), len(G.FAMILIES)
    Eo, En = np.full((nr, nf, 4), np.nan), np.full((nr, nf, 4), np.nan)
    po = fx["family"] == G.FAMILIES.index("prediction_only")
    for ri, D in enumerate(doubles):
        for fi in range(len(G.SINGLE)):
            cs = np.nonzero((fx["regime"] == ri) & (fx["family"] == fi))[0]
            Eo[ri, fi] = np.max([errors(D.oracle(*_case(fx, c), prediction=bool(po[c])), _ref(fx, c)) for c in cs], axis=0)
            En[ri, fi] = np.max([errors(D.numpy(*_case(fx, c), prediction=bool(po[c])), _ref(fx, c)) for c in cs], axis=0)
    fi = G.FAMILIES.index("chain")
    for ci, ri in enumerate(fx["chain_regime"]):
        D = doubles[ri]
        eo, en = [], []
        for b in range(G.CHAIN_FILTERS):
            xo, Po = fx["chain_x0"][b], from_triu(fx["chain_P0u"][b])
            xn, Pn = xo, Po
            for k in range(G.CHAIN_TICKS):
                a = (fx["chain_thrust"][ci, k, b], fx["chain_y12"][ci, k, b], fx["chain_acc"][ci, k, b])
                ref = (fx["chain_xn"][ci, k, b], from_triu(fx["chain_Pnu"][ci, k, b]), fx["chain_wf"][ci, k, b], fx["chain_mp"][ci, k, b])
                o = D.oracle(xo, Po, *a); xo, Po = o[0], o[1]
                n = D.numpy(xn, Pn, *a); xn, Pn = n[0], n[1]
                eo.append(errors(o, ref)); en.append(errors(n, ref))
        Eo[ri, fi], En[ri, fi] = np.max(eo, axis=0), np.max(en, axis=0)
    for got, want, name in ((Eo, fx["E_orc"], "E_orc"), (En, fx["E_np"], "E_np")):
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = np.isnan(want) | ((np.maximum(got, FLOOR) <= FACTOR * np.maximum(want, FLOOR)) & (np.maximum(want, FLOOR) <= FACTOR * np.maximum(got, FLOOR)))
        assert ok.all(), (name, np.argwhere(~ok), got[~ok], want[~ok])
    print(f"[ekf_exact] stored E reproduced exactly: E_orc {np.array_equal(Eo, fx['E_orc'], equal_nan=True)}, E_np {np.array_equal(En, fx['E_np'], equal_nan=True)}")
    # what the bars come to: the tight regime's single ticks in the 1e-12 range or below but for the scaled covariances, the shipped regime's at 1e-8
    t, s = G.REGIMES.index("tight"), G.REGIMES.index("shipped")
    E = np.fmax(fx["E_orc"], fx["E_np"])
    cov = G.FAMILIES.index("cov_scaled")
    assert np.nanmax(np.delete(E[t], cov, axis=0)) < 3e-12 and np.nanmax(E[t]) < 3e-11, E[t]
    assert 1e-9 < np.nanmax(E[s]) < 1e-7, E[s]


def test_cases_meet_their_conditions_on_the_reference_alone(fx):
    fam, reg = fx["family"], fx["regime"]
    po = fam == G.FAMILIES.index("prediction_only")
    assert np.all(fx["piv_min"][~po] > 0) and np.all(fx["status"][~po] == 0)                   # S positive definite: no row exchange needed
    assert np.all(fx["piv_first"][po] < 0) and np.all(fx["status"][po] == 1)
    assert np.all(fx["chain_piv_min"] > 0)
    assert np.all(np.linalg.eigvalsh(from_triu(fx["P0u"][fx["in_family"] == G.FAMILIES.index("prediction_only")])) < -0.4)   # P = -(A A' + I / 2)
    for a in (fx["x0"][:, 3:6], fx["y12"][:, 3:6], fx["xn"][:, 3:6], fx["chain_y12"][..., 3:6], fx["chain_xn"][..., 3:6]):
        assert np.abs(a).max() <= TRIG_DOMAIN
    assert np.abs(fx["xn"][:, 3:5]).max() < 1.3 and np.abs(fx["y12"][:, 3:5]).max() < 1.3                    # away from cos(theta) = 0
    # every family in every regime it is meant for, with the generator's counts
    for ri, r in enumerate(G.REGIMES):
        for fi in range(len(G.SINGLE)):
            assert ((reg == ri) & (fam == fi)).sum() == G.COUNT[r] >= 2, (r, fi)
            assert np.array_equal(fx["in_family"][fx["input"][(reg == ri) & (fam == fi)]], np.full(G.COUNT[r], fi))
        has_chain = r in G.CHAIN_REGIMES
        assert np.isfinite(fx["E_orc"][ri, -1]).all() == has_chain and np.isfinite(fx["E_np"][ri, -1]).all() == has_chain
        assert np.isfinite(fx["E_orc"][ri, :-1]).all() and np.isfinite(fx["E_np"][ri, :-1]).all()
    assert [G.REGIMES[i] for i in fx["chain_regime"]] == list(G.CHAIN_REGIMES) and fx["chain_xn"].shape == (2, 6, 3, 18)
    # the families are what they say
    x0, inf = fx["x0"], fx["in_family"]
    f = G.FAMILIES.index
    assert not x0[inf == f("zero_motion"), 3:12].any() and not x0[inf == f("zero_dist"), 12:18].any()
    far = x0[inf == f("far_yaw")]
    assert np.abs(far[:, 5]).min() >= 200 and np.abs(far[:, 3:5]).max() == 1.0 and (far[:, 3:5] == -1.0).any()
    scale = np.abs(from_triu(fx["P0u"][inf == f("cov_scaled")])).max(axis=(1, 2))
    assert scale.min() < 1e-5 and scale.max() > 10 and scale[:2].min() < 1e-5 and scale[:2].max() > 10      # both ends in every regime
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ekf_exact.npz")) < 350 * 1024


# ---- the bar has teeth ---------------------------------------------------------------------------------------------------------------------------
MISTAKES = ("third stage at k2/2", "R K K' dropped", "F[9][16] zeroed", "H[14][3] zeroed", "H[17][11] zeroed", "Q[17] := Q[16]",
            "R left off S[17][17]", "columns 16, 17 of F exchanged")


def _update_with(mistake):
    """test_oracle_ekf.np_update, statement by statement, with one deliberate mistake (None: none -- checked to be np_update bit for bit)"""
    def rk4(c, x, tau):
        if mistake != "third stage at k2/2":
            return T.np_rk4(c, x, tau)
        dt = c["dt"]
        k1 = T.np_f(c, x, tau) * dt
        k2 = T.np_f(c, x + k1 / 2, tau) * dt
        k3 = T.np_f(c, x + k2 / 2, tau) * dt
        k4 = T.np_f(c, x + k3, tau) * dt
        return x + (k1 + 2 * k2 + 2 * k3 + k4) / 6

    def update(c, x, P, thrust, y12, acc):
        tau = c["K"] @ thrust
        y = np.concatenate([y12, tau])
        F = T.np_fd(lambda z: rk4(c, z, tau), x, c["fd_step"])
        if mistake == "F[9][16] zeroed":
            F[9, 16] = 0.0
        if mistake == "columns 16, 17 of F exchanged":
            F[:, [16, 17]] = F[:, [17, 16]]
        xp = rk4(c, x, tau)
        Q = c["Q"].copy()
        if mistake == "Q[17] := Q[16]":
            Q[17] = Q[16]
        Pp = F @ P @ F.T + np.diag(Q)
        H = T.np_fd(lambda z: T.np_h(c, z, acc), xp, c["fd_step"])
        if mistake == "H[14][3] zeroed":
            H[14, 3] = 0.0
        if mistake == "H[17][11] zeroed":
            H[17, 11] = 0.0
        ye = y - T.np_h(c, xp, acc)
        Rm = np.eye(18) * c["R"]
        S = H @ Pp @ H.T + Rm
        if mistake == "R left off S[17][17]":
            S[17, 17] = (H @ Pp @ H.T)[17, 17]
        Kal = Pp @ H.T @ np.linalg.inv(S)
        xn = xp + Kal @ ye
        J = np.eye(18) - Kal @ H
        Pn = J @ Pp @ J.T
        if mistake != "R K K' dropped":
            Pn = Pn + Kal @ Rm @ Kal.T
        return xn, Pn
    return update


def _today_lets_through(got, ref):
    """the tolerances of tests/test_gpu_ekf.test_single_tick_vs_oracle"""
    return (np.allclose(got[0], ref[0], rtol=1e-6, atol=1e-6) and np.allclose(got[1], ref[1], rtol=1e-5, atol=1e-7) and
            np.allclose(got[2], ref[2], rtol=1e-6, atol=1e-6) and np.allclose(got[3], ref[3], rtol=1e-6, atol=1e-4))


def test_the_bar_has_teeth(fx, doubles):
    """each mistake, made in the numpy restatement, exceeds 4 x max(E_orc, E_np, 2^-50) of the tight regime on at least one quantity of at
    least one family by a factor of 100 or more; and which of them the shipped regime's cases pass at today's tolerances"""
    t, s = G.REGIMES.index("tight"), G.REGIMES.index("shipped")
    po = G.FAMILIES.index("prediction_only")
    E = np.fmax(np.fmax(fx["E_orc"], fx["E_np"]), FLOOR)
    cases = {ri: np.nonzero((fx["regime"] == ri) & (fx["family"] != po))[0] for ri in (t, s)}
    plain = _update_with(None)
    for c in cases[t][:3]:
        a, b = plain(doubles[t].c, *_case(fx, c)), T.np_update(doubles[t].c, *_case(fx, c))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    lines, missed = [], []
    for mistake in MISTAKES:
        upd = _update_with(mistake)
        ratio = np.zeros(4)
        for c in cases[t]:
            e = errors(doubles[t].numpy(*_case(fx, c), update=upd), _ref(fx, c))
            ratio = np.maximum(ratio, e / (FACTOR * E[t, fx["family"][c]]))
        through = all(_today_lets_through(doubles[s].numpy(*_case(fx, c), update=upd), _ref(fx, c)) for c in cases[s])
        worst_today = np.max([errors(doubles[s].numpy(*_case(fx, c), update=upd), _ref(fx, c)) for c in cases[s]], axis=0)
        lines.append(f"{mistake:32s} tight: error / bar " + " ".join(f"{q} {v:.1e}" for q, v in zip(QUANTITIES, ratio)) +
                     f";  shipped at 1e-6 / 1e-5: {'PASSES (let through)' if through else 'caught'} (scaled errors " +
                     " ".join(f"{v:.1e}" for v in worst_today) + ")")
        if not ratio.max() >= 100.0:
            missed.append((mistake, ratio))
        if mistake == "Q[17] := Q[16]":     # invisible by construction with the default Q: the same bits
            for c in cases[s][:4]:
                a, b = upd(doubles[s].c, *_case(fx, c)), plain(doubles[s].c, *_case(fx, c))
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and through
    print("\n[ekf_exact] deliberate mistakes in the numpy restatement\n" + "\n".join(lines))
    path = os.environ.get("BROV_EKF_EXACT_TEETH_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert not missed, missed
