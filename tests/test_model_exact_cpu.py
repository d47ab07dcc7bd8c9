"""The 60-digit model (tests/model_exact.py) and its fixture (tests/golden/model_exact.npz, scripts/make_model_exact_golden.py), checked
without a GPU: the new reference against the reference project's own CasADi vectors, the fixture against a recomputation, and the
double-precision oracle against the fixture -- the bar the GPU tests hold the device to (tests/test_gpu_model_exact.py) is one a correct
double implementation meets on every case."""
import os

import numpy as np
import pytest

from model_exact import ExactModel, LongDoubleBackend, MpBackend, scaled_err
from wrench_restatement import f_under_wrench, rk4_under_wrench

RTOL = 1e-12      # the bound of tests/test_oracle_model.py
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_exact.npz")


def _rel(a, b):
    return np.abs(a - b).max() / (1.0 + np.abs(b).max())


@pytest.fixture(scope="module")
def exact():
    return ExactModel(MpBackend())


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


def test_exact_model_reproduces_the_reference_vectors(exact, golden_model):
    """f, A, B and one ERK4 step with sensitivities at three step sizes, from the reference's CasADi C: pins the new yardstick itself"""
    g = golden_model
    for t in range(0, g["x"].shape[0], 4):
        x, u, p = g["x"][t], g["u"][t], g["p"][t]
        assert _rel(exact.f_double(x, u, p), g["f"][t]) < RTOL
        J = exact.jac(x, u, p)
        assert _rel(J[:, :12], g["A"][t]) < RTOL and _rel(J[:, 12:], g["B"][t]) < RTOL
    for ih, h in enumerate(g["h"]):
        for t in range(ih, g["xn"].shape[1], 8):
            xn, S = exact.sens(g["x"][t], g["u"][t], g["p"][t], float(h))
            assert _rel(xn, g["xn"][ih, t]) < RTOL
            assert _rel(S[:, :12], g["Ad"][ih, t]) < RTOL and _rel(S[:, 12:], g["Bd"][ih, t]) < RTOL


def test_fixture_is_what_the_exact_model_gives_bit_for_bit(exact, fx):
    fam = fx["family"]
    names = list(fx["families"])
    wf, d6 = names.index("world_wrench"), names.index("dist6")
    for c in range(0, len(fam), 7):
        x, u, p, h = fx["x"][c], fx["u"][c], fx["p"][c], float(fx["h"][c])
        ww, rp = (fx["ww"][c] if fam[c] == wf else None), (fx["rp"][c] if fam[c] == d6 else None)
        assert np.array_equal(exact.f_double(x, u, p, ww, rp), fx["f"][c]), c
        if fam[c] == wf:
            assert np.array_equal(exact.erk4(x, u, p, h, ww), fx["xn"][c]), c
        else:
            xn, S = exact.sens(x, u, p, h, None, rp)
            assert np.array_equal(xn, fx["xn"][c]) and np.array_equal(S, fx["S"][c]), c


def test_fixture_covers_what_it_says(fx):
    names = list(fx["families"])
    assert names == ["wide", "quadrant_edges", "kinks", "far_yaw", "steep_pitch", "parameters", "world_wrench", "dist6"]
    fam, x, p = fx["family"], fx["x"], fx["p"]
    assert set(np.unique(fx["h"])) == {0.0125, 0.05, 0.1} and np.bincount(fam).max() <= 64
    assert np.abs(fx["u"]).max() <= 50.0
    at_bound = (np.abs(fx["u"]) == 50.0).any(axis=1)
    assert all(at_bound[fam == fi].sum() >= 2 for fi in range(len(names))), np.bincount(fam[at_bound], minlength=len(names))
    q = x[fam == names.index("quadrant_edges")]
    k = np.rint(q[:, 5] / (np.pi / 2)).astype(int)
    on_axis = np.abs(q[:, 5] - k * (np.pi / 2)) < 1e-9
    assert {(int(v) % 4, int(np.sign(v))) for v in k[on_axis]} == {(r, s) for r in range(4) for s in (-1, 1)}
    assert np.abs(q[:, 5]).max() > 390 and np.abs(q[:, 4]).max() < 0.8
    kk = x[fam == names.index("kinks")][:, [6, 7, 8, 11]]
    assert (kk == 0.0).any() and (np.signbit(kk) & (kk == 0.0)).any() and (np.abs(kk) == 1e-300).any()
    assert np.abs(x[fam == names.index("far_yaw"), 5]).max() > 3e4
    st = np.abs(x[fam == names.index("steep_pitch"), 4])
    assert st.min() >= 1.3 and st.max() <= 1.5
    pp = p[fam == names.index("parameters")]
    assert (11.26 + pp[:, 4:7]).min() <= 1.0 + 1e-12 and (11.26 + pp[:, 4:7]).max() >= 50.0 - 1e-9
    assert (pp[:, 8:12] == 0).all(axis=1).any() and (pp[:, 12:16] == 0).all(axis=1).any()
    assert np.abs(fx["ww"][fam == names.index("world_wrench")]).max() > 250 and not fx["ww"][fam != names.index("world_wrench")].any()
    assert np.abs(fx["rp"][fam == names.index("dist6")]).max() > 4 and not fx["rp"][fam != names.index("dist6")].any()


def test_oracle_stays_within_its_stored_error_on_every_case(oracle, fx):
    """E_orc, the per-family bar of the GPU tests, is met by a plain double implementation on every case, none left out"""
    fam = fx["family"]
    names = list(fx["families"])
    wf = names.index("world_wrench")
    for c in range(len(fam)):
        x, u, p, h, ww, rp = fx["x"][c], fx["u"][c], fx["p"][c], float(fx["h"][c]), fx["ww"][c], fx["rp"][c]
        E = fx["E_orc"][fam[c]]
        if fam[c] == wf:
            of, oxn = f_under_wrench(oracle, x, u, p, ww), rk4_under_wrench(oracle, x, u, p, ww, h)
        else:
            of = oracle.f6(x, u, p, rp)
            oxn, oA, oB = oracle.rk4_sens(x, u, p, h, drp=rp if rp.any() else None)
            eS = scaled_err(np.concatenate([oA, oB], axis=1), fx["S"][c]).max()
            assert eS <= E[2], (c, eS)
        ef, ex = scaled_err(of, fx["f"][c]).max(), scaled_err(oxn, fx["xn"][c]).max()
        assert ef <= E[0] and ex <= E[1], (c, ef, ex)
    # a double implementation's rounding on well-conditioned steps, with the one family whose stage points round at |psi| ~ 1e5 apart
    far = names.index("far_yaw")
    assert np.nanmax(np.delete(fx["E_orc"], far, axis=0)) < 2e-13 and np.nanmax(fx["E_orc"][far]) < 5e-12


def test_position_columns_of_the_exact_sensitivities_are_the_identity_block(fx):
    S = fx["S"][fx["family"] != list(fx["families"]).index("world_wrench")]
    assert np.array_equal(S[:, :, :3], np.broadcast_to(np.eye(12)[:, :3], (len(S), 12, 3)))


def test_longdouble_backend_agrees_with_mpmath_on_f_and_the_step(exact, fx):
    """the fall-back reference of the run-time GPU cases, where mpmath cannot be imported"""
    if np.finfo(np.longdouble).nmant < 63:
        with pytest.raises(RuntimeError):
            LongDoubleBackend()
        return
    L = ExactModel(LongDoubleBackend())
    for c in range(0, len(fx["h"]), 5):
        x, u, p, h, ww, rp = fx["x"][c], fx["u"][c], fx["p"][c], float(fx["h"][c]), fx["ww"][c], fx["rp"][c]
        # both are rounded to double (one ulp between them at most: 2^-52 scaled); the long double's own rounding, 2^-64 relative
        # per operation at the size of the largest entry (the yaw angle of the stage points), over a few tens of operations: 2^-60 |x|
        tol = 2.0 ** -52 + 2.0 ** -60 * max(1.0, np.abs(x).max())
        assert scaled_err(L.f_double(x, u, p, ww, rp), exact.f_double(x, u, p, ww, rp)).max() <= tol
        assert scaled_err(L.erk4(x, u, p, h, ww, rp, substeps=4), exact.erk4(x, u, p, h, ww, rp, substeps=4)).max() <= tol
