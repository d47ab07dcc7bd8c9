"""ekf_update_kernel_sp, every tick, against the same filter carried out at 60 digits (tests/ekf_exact.py; fixture tests/golden/ekf_exact.npz,
scripts/make_ekf_exact_golden.py).  This file reads the fixture only.

Why.  tests/test_gpu_ekf.py holds the kernel to the double oracle at 1e-6 / 1e-5, which is what two correct FP64 evaluations of the SHIPPED
parameters agree to (fd_step = 1e-6 and an innovation covariance of condition 1e9 amplify last-bit differences) -- and two to seven orders
wider than a dropped Jacobian entry, a wrong Q index or a wrong symmetric fill needs to hide in.  fd_step, R and Q are ordinary fields of
brov_ekf_params: the same kernel, instruction stream and zero pattern run here in regimes (tight: fd_step 2^-7, R 1; mid: 2^-10, 1e-2; Q of 18
pairwise different entries) where two correct evaluations agree to 1e-13, besides the shipped one.

The bar.  Errors are scaled: x, wf, mpc_p |got - ref| / max(1, |ref|) per entry, P |got - ref| / max |ref| per filter.  Per regime, family and
quantity the device's error must be <= 4 x max(E_orc, E_np, 2^-50): E_orc, E_np are the worst errors of the C oracle and of the numpy
restatement test_oracle_ekf.np_update on the same family against the SAME reference, stored with the fixture -- never an error measured on the
device.  The factor 4 and the floor are those of tests/test_gpu_model_exact.py, for the same reasons (trig good to 1.5 ulp, Newton reciprocals,
another order of FMA contraction) and one more: elimination without pivoting against the oracle's pivoted LU.  No case is excused.
One regime and family (WIDER) may add, on a case that misses this, the first-order bound of what rounding the forward differences does,
computed with the fixture: the cause and the share of the bound used stand beside the figures.

The figures of a run are printed (pytest -s) and, with BROV_EKF_EXACT_REPORT=<file> set, written there (profiles/ekf_exact.txt is a copy)."""
import os

import numpy as np
import pytest

from ekf_exact import QUANTITIES, err_P, err_x, from_triu, par_apply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR, FLOOR = 4.0, 2.0 ** -50
REGIMES = ("shipped", "tight", "mid", "device_loop", "varied")
_MEASURED = {}
_BATCH = {}


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


@pytest.fixture(scope="module")
def fx():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ekf_exact.npz"))
    d = {k: g[k] for k in g.files}
    d["regime_names"], d["family_names"] = list(d["regimes"]), list(d["families"])
    assert tuple(d["regime_names"]) == REGIMES and tuple(d["quantities"]) == QUANTITIES
    return d


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("BROV_EKF_EXACT_REPORT")
    if not _MEASURED or not path:
        return
    with open(path, "w") as f:
        f.write("EKF observer kernel against the 60-digit filter (tests/test_gpu_ekf_exact.py)\n"
                "per regime, family and quantity: the device's worst scaled error (the C oracle's E_orc, the numpy restatement's E_np, "
                "ratio = device / max(E_orc, E_np, 2^-50)); the bar is a ratio of 4\n\n")
        for k in sorted(_MEASURED):
            f.write(f"{k}: {_MEASURED[k]}\n")


def _note(key, text):
    _MEASURED[key] = text
    print(f"[ekf_exact] {key}: {text}")


def _bar(fx, ri, fi, q):
    return FACTOR * max(float(fx["E_orc"][ri, fi, q]), float(fx["E_np"][ri, fi, q]), FLOOR)      # (a NaN E: no such family in this regime -- fails)


# A (regime, family) whose ticks may miss the plain bar for a reason that is conditioning, not the kernel: the cause, and beside the figure the
# share of the first-order bound used (fx["fd_bound"]: ekf_exact.fd_rounding_bound at the case's own inputs, computed by the fixture's generator
# from the restatement's F, H and S -- what rounding the two forward differences can do to the outputs; nothing measured on the device).
WIDER = {
    ("shipped", "zero_motion"):
        "fd_step = 1e-6 turns a rounding of the RK4 map or of h (1e-16 of the terms summed) into 1e-10 of an entry of F or H, and S (R = 1.6e-6, "
        "condition 1e9) carries that into the gain.  With angles, velocities and rates at 0 the two double implementations happen to come within "
        "8e-10 on the six cases (every other shipped family: 3e-9 .. 4e-8), and mpc_p = x / 0.03 shows a disturbance estimate below 1 thirty times "
        "larger than the scaled x does: one case's mpc_p sits at 4.5 E.  The same instruction stream meets the plain bar in the tight regime "
        "(ratio 1.3), and the prediction alone does here (0.6).",
}


def _hold(what, fx, ri, fam, dev, quantities=range(4), bar_family=None, bound=None):
    """dev [cases, 4]: the device's scaled error of every case for x, P, wf, mpc_p; fam [cases].  Every case of every family within
    FACTOR x max(E_orc, E_np, FLOOR) of its regime, family (bar_family: that family's bar instead) and quantity; the ratios are recorded first.
    A case of a (regime, family) in WIDER that misses this has its own first-order bound (bound [cases, 4]) added; no other has, none is left out."""
    dev, fam = np.asarray(dev), np.asarray(fam)
    parts, bad = [], []
    for fi in np.unique(fam):
        bf = fi if bar_family is None else bar_family
        wider = bound is not None and (REGIMES[ri], fx["family_names"][fi]) in WIDER
        for q in quantities:
            bar = _bar(fx, ri, bf, q)
            e = dev[fam == fi, q]
            worst = float(np.max(e))
            text = (f"{fx['family_names'][fi]} {QUANTITIES[q]} {worst:.2e} (oracle {float(fx['E_orc'][ri, bf, q]):.2e}, numpy "
                    f"{float(fx['E_np'][ri, bf, q]):.2e}, ratio {worst / (bar / FACTOR):.2f}")
            over = ~(e <= bar)      # (a NaN is over)
            if over.any() and wider:
                b = np.asarray(bound)[fam == fi, q]
                used = float(np.max((e[over] - bar) / b[over]))
                text += f"; {int(over.sum())} of {len(e)} cases over the plain bar, at most {used:.3f} of their first-order rounding bound"
                if not np.all(e[over] <= bar + b[over]):
                    bad.append((fx["family_names"][fi], QUANTITIES[q], worst, bar, b[over]))
            elif over.any():
                bad.append((fx["family_names"][fi], QUANTITIES[q], worst, bar))
            parts.append(text + ")")
    _note(what, "; ".join(parts))
    assert not bad, (what, bad)


def _params(ba, vec):
    return par_apply(ba.EkfParams.default(), vec)


def _tick(ba, par, x, P, thrust, y12, acc):
    e = ba.BatchEkf(len(x), par)
    e.set_state(x, P); e.update(thrust, y12, acc)
    out = e.state() + e.outputs()
    e.close()
    return out          # x, P, wf, mpc_p, status


def _regime(fx, ri):
    """the single ticks of a regime: (rows of the fixture, family, x, P, thrust, y12, acc)"""
    idx = np.nonzero(fx["regime"] == ri)[0]
    return idx, fx["family"][idx], fx["x0"][fx["input"][idx]], from_triu(fx["P0u"][fx["input"][idx]]), fx["thrust"][idx], fx["y12"][idx], fx["acc"][idx]


def _regime_outputs(ba, fx, ri):
    """... and what the device makes of them in ONE batch (computed once: the other tests compare with it bit for bit)"""
    if ri not in _BATCH:
        idx, fam, x, P, thrust, y12, acc = _regime(fx, ri)
        _BATCH[ri] = _tick(ba, _params(ba, fx["par"][ri]), x, P, thrust, y12, acc)
    return _BATCH[ri]


def _errors(out, xr, Pr, wfr, mpr):
    with np.errstate(invalid="ignore"):
        return np.stack([err_x(out[0], xr), err_P(out[1], Pr), err_x(out[2], wfr), err_x(out[3], mpr)], axis=1)


# ---- 1. single ticks, one batch per regime ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
def test_single_ticks_of_every_family(ba, fx, regime):
    """B = the regime's case count (a few dozen: several waves).  Every family but prediction_only: status 0.  prediction_only: P = -(A A' + I / 2),
    the first pivot of S is negative -- status 1 on every case, x and P held to the bar against x_pred and P_pred = F P F' + Q, P exactly
    symmetric: F, G = P F', F G + Q and the symmetric fill, apart from the gain and the Joseph form."""
    ri = REGIMES.index(regime)
    idx, fam, x, P, thrust, y12, acc = _regime(fx, ri)
    out = _regime_outputs(ba, fx, ri)
    only = fam == fx["family_names"].index("prediction_only")
    assert len(idx) >= 12 and only.sum() >= 2 and len(np.unique(fam)) == 6
    assert np.array_equal(out[4], only.astype(np.int32)), out[4]
    assert np.array_equal(fx["status"][idx], out[4])
    asym = np.abs(out[1] - np.swapaxes(out[1], 1, 2)).max(axis=(1, 2)) / np.abs(out[1]).max(axis=(1, 2))
    _note(f"1 {regime} symmetry", f"worst |P - P'| / max |P|: prediction_only {asym[only].max():.2e}, the other families {asym[~only].max():.2e}")
    _hold(f"1 {regime} single ticks (B = {len(idx)})", fx, ri, fam, _errors(out, fx["xn"][idx], from_triu(fx["Pnu"][idx]), fx["wf"][idx], fx["mp"][idx]),
          bound=fx["fd_bound"][idx])
    assert np.array_equal(out[1][only], np.swapaxes(out[1][only], 1, 2)), asym[only]


@pytest.mark.parametrize("regime", REGIMES)
def test_rotated_batches_are_bit_identical(ba, fx, regime):
    """the same cases rotated by 1, 2 and 3 positions: every case sits in each of a wave's four 16-lane rows"""
    ri = REGIMES.index(regime)
    idx, fam, x, P, thrust, y12, acc = _regime(fx, ri)
    ref = _regime_outputs(ba, fx, ri)
    par = _params(ba, fx["par"][ri])
    for s in (1, 2, 3):
        out = _tick(ba, par, *(np.roll(a, s, axis=0) for a in (x, P, thrust, y12, acc)))
        for a, b in zip(out, ref):
            assert np.array_equal(np.roll(a, -s, axis=0), b), (regime, s)


@pytest.mark.parametrize("regime", ["tight", "shipped"])
def test_one_filter_alone_and_a_tail_wave_with_one_live_filter(ba, fx, regime):
    """B = 1 (three of the wave's four rows idle) and B = 4 k + 1 (the last wave has one live filter): bit for bit what the full batch gives,
    which test_single_ticks_of_every_family holds to the bar"""
    ri = REGIMES.index(regime)
    idx, fam, x, P, thrust, y12, acc = _regime(fx, ri)
    ref = _regime_outputs(ba, fx, ri)
    par = _params(ba, fx["par"][ri])
    n = 4 * ((len(idx) - 1) // 4) + 1
    assert n % 4 == 1 and n >= 13
    out = _tick(ba, par, x[:n], P[:n], thrust[:n], y12[:n], acc[:n])
    for a, b in zip(out, ref):
        assert np.array_equal(a, b[:n]), regime
    far = int(np.nonzero(fam == fx["family_names"].index("far_yaw"))[0][0])
    for c in (n - 1, far):
        out = _tick(ba, par, x[c:c + 1], P[c:c + 1], thrust[c:c + 1], y12[c:c + 1], acc[c:c + 1])
        for a, b in zip(out, ref):
            assert np.array_equal(a, b[c:c + 1]), (regime, c)


# ---- 2. chains: the device carries its own state ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1])
def test_chain_of_six_ticks(ba, fx, ci):
    """3 filters x 6 ticks: the reference carried its state at 60 digits, the double implementations theirs in double (their errors at every
    tick are the family's E); the device carries its own and is held at EVERY tick"""
    ri = int(fx["chain_regime"][ci])
    fi = fx["family_names"].index("chain")
    K, B = fx["chain_xn"].shape[1:3]
    e = ba.BatchEkf(B, _params(ba, fx["par"][ri]))
    e.set_state(fx["chain_x0"], from_triu(fx["chain_P0u"]))
    dev = []
    for k in range(K):
        e.update(fx["chain_thrust"][ci, k], fx["chain_y12"][ci, k], fx["chain_acc"][ci, k])
        out = e.state() + e.outputs()
        assert not out[4].any(), (k, out[4])
        dev.append(_errors(out, fx["chain_xn"][ci, k], from_triu(fx["chain_Pnu"][ci, k]), fx["chain_wf"][ci, k], fx["chain_mp"][ci, k]))
    e.close()
    dev = np.array(dev)         # [ticks, filters, quantities]
    _note(f"2 {REGIMES[ri]} chain, worst x per tick", " ".join(f"{v:.2e}" for v in dev[:, :, 0].max(axis=1)))
    _hold(f"2 {REGIMES[ri]} chain ({B} filters x {K} ticks)", fx, ri, np.full(K * B, fi), dev.reshape(K * B, 4))


# ---- 3. the documented NaN cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
def test_nan_acceleration_leaves_the_prediction_and_nan_measurement_is_flagged(ba, fx, regime):
    """acc[., 2] = NaN: h's base evaluation and with it S hold a NaN -- status 1, and the header's promise for it: estimate and covariance left
    at the prediction (x_pred, P_pred of the reference, which do not depend on acc), held to the bar of the case's regime and family; wf and
    mpc_p finite.  y12 = NaN: status 2, the estimate not finite.  The other filters of the batch: bit for bit what they are without the two."""
    ri = REGIMES.index(regime)
    idx, fam, x, P, thrust, y12, acc = _regime(fx, ri)
    ref = _regime_outputs(ba, fx, ri)
    k = int(np.nonzero(fx["pred_case"] == idx[0])[0][0])      # the regime's first case: nominal, its prediction stored
    assert fam[0] == fx["family_names"].index("nominal") and ref[4][0] == 0
    a_nan, y_nan = 0, 6                                       # wave 0, row 0 (rows 1..3: live neighbours); wave 1, row 2
    assert ref[4][y_nan] == 0
    acc, y12 = acc.copy(), y12.copy()
    acc[a_nan, 2] = np.nan
    y12[y_nan, 0] = np.nan
    out = _tick(ba, _params(ba, fx["par"][ri]), x, P, thrust, y12, acc)
    xg, Pg, wfg, mpg, st = out
    others = np.ones(len(idx), dtype=bool); others[[a_nan, y_nan]] = False
    for a, b in zip(out, ref):
        assert np.array_equal(a[others], b[others]), regime
    assert st[a_nan] == 1 and st[y_nan] == 2 and not np.isfinite(xg[y_nan]).all()
    _note(f"3 {regime} NaN acceleration", f"status {st[a_nan]}, x finite {bool(np.isfinite(xg[a_nan]).all())}, P finite {bool(np.isfinite(Pg[a_nan]).all())}, "
          f"wf finite {bool(np.isfinite(wfg[a_nan]).all())}, mpc_p finite {bool(np.isfinite(mpg[a_nan]).all())}")
    dev = np.zeros((1, 4))
    with np.errstate(invalid="ignore"):
        dev[0, 0], dev[0, 1] = err_x(xg[a_nan], fx["pred_x"][k]), err_P(Pg[a_nan], from_triu(fx["pred_Pu"][k]))
    _hold(f"3 {regime} NaN acceleration against the prediction", fx, ri, fam[:1], dev, quantities=(0, 1))
    assert np.isfinite(wfg[a_nan]).all() and np.isfinite(mpg[a_nan]).all()
