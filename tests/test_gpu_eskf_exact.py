"""eskf_tick_kernel, every tick, against the same filter carried out at 60 digits (tests/eskf_exact.py; fixture tests/golden/eskf_exact.npz,
scripts/make_eskf_exact_golden.py).  This file reads the fixture only.

The bar, as in tests/test_gpu_ekf_exact.py.  Errors are scaled: x, xi_world, mpc_p |got - ref| / max(1, |ref|) per entry (a quaternion compared up
to sign), P |got - ref| / max |ref| per filter.  Per regime, family and quantity the device's error must be <= 4 x max(E_np, 2^-50): E_np is the
worst error of the numpy restatement on the same family against the SAME reference, stored with the fixture -- never an error measured on the
device.  The factor 4 and the floor are that file's, for its reasons: trig good to 1.5 ulp, reciprocals, another order of FMA contraction,
elimination without exchanges as L D L' here and as Gauss-Jordan there.  No case is excused and there is no list of wider cases.

The figures of a run are printed (pytest -s) and, with BROV_ESKF_EXACT_REPORT=<file> set, written there (profiles/eskf_exact.txt is a copy)."""
import os

import numpy as np
import pytest

from eskf_exact import QUANTITIES, err_P, err_state, err_x, from_triu, par_apply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR, FLOOR = 4.0, 2.0 ** -50
REGIMES = ("shipped", "varied", "loop")
FILTERS_PER_WAVE = 2
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
    g = np.load(os.path.join(ROOT, "tests", "golden", "eskf_exact.npz"))
    d = {k: g[k] for k in g.files}
    d["regime_names"], d["family_names"] = list(d["regimes"]), list(d["families"])
    assert tuple(d["regime_names"]) == REGIMES and tuple(d["quantities"]) == QUANTITIES
    return d


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("BROV_ESKF_EXACT_REPORT")
    if not _MEASURED or not path:
        return
    with open(path, "w") as f:
        f.write("Error-state filter kernel against the 60-digit filter (tests/test_gpu_eskf_exact.py)\n"
                "per regime, family and quantity: the device's worst scaled error (the numpy restatement's E_np, ratio = device / max(E_np, 2^-50)); "
                "the bar is a ratio of 4\n\n")
        for k in sorted(_MEASURED):
            f.write(f"{k}: {_MEASURED[k]}\n")


def _note(key, text):
    _MEASURED[key] = text
    print(f"[eskf_exact] {key}: {text}")


def _hold(what, fx, ri, fam, dev):
    """dev [cases, 4]: the device's scaled error of every case for x, P, xi_world, mpc_p; fam [cases].  Every case of every family within
    FACTOR x max(E_np, FLOOR) of its regime, family and quantity; the ratios are recorded first"""
    dev, fam = np.asarray(dev), np.asarray(fam)
    parts, bad = [], []
    for fi in np.unique(fam):
        for q in range(4):
            e_np = float(fx["E_np"][ri, fi, q])
            bar = FACTOR * max(e_np, FLOOR)      # (a NaN E: no such family in this regime -- fails)
            worst = float(np.max(dev[fam == fi, q]))
            parts.append(f"{fx['family_names'][fi]} {QUANTITIES[q]} {worst:.2e} (numpy {e_np:.2e}, ratio {worst / (bar / FACTOR):.2f})")
            if not worst <= bar:
                bad.append((fx["family_names"][fi], QUANTITIES[q], worst, bar))
    _note(what, "; ".join(parts))
    assert not bad, (what, bad)


def _params(ba, vec):
    return par_apply(ba.EskfParams.default(), vec)


def _tick(ba, par, x, P, imu, gps_p, gps_v, qm, thrust, update=True):
    e = ba.BatchEskf(len(x), par)
    e.set_state(x, P)
    if update:
        e.update(imu, gps_p, gps_v, qm, thrust)
    else:
        e.predict(imu)
    out = e.state() + e.outputs()
    e.close()
    return out          # x, P, xi, xi_world, mpc_p, status


def _regime(fx, ri, update):
    """the single ticks of a regime that are update ticks (or the predict-only ones): (rows of the fixture, family, the tick's arguments)"""
    po = fx["family_names"].index("predict_only")
    idx = np.nonzero((fx["regime"] == ri) & ((fx["family"] != po) == update))[0]
    return idx, fx["family"][idx], (fx["x0"][idx], from_triu(fx["P0u"][fx["input"][idx]]), fx["imu"][idx], fx["gps_p"][idx], fx["gps_v"][idx],
                                    fx["qm"][idx], fx["thrust"][idx])


def _regime_outputs(ba, fx, ri, update):
    """... and what the device makes of them in ONE batch (computed once: the other tests compare with it bit for bit)"""
    if (ri, update) not in _BATCH:
        idx, fam, args = _regime(fx, ri, update)
        _BATCH[ri, update] = _tick(ba, _params(ba, fx["par"][ri]), *args, update=update)
    return _BATCH[ri, update]


def _errors(out, xr, Pr, xwr, mpr):
    with np.errstate(invalid="ignore"):
        return np.stack([err_state(out[0], xr), err_P(out[1], Pr), err_x(out[3], xwr), err_x(out[4], mpr)], axis=1)


# ---- 1. single ticks, one batch per regime and entry shape -----------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
def test_single_ticks_of_every_family(ba, fx, regime):
    """the update ticks of a regime as one batch (17 filters: nine waves, the last with one live filter) and its predict-only ticks as another.
    prediction_left: P = -(A A' + I / 2), the first pivot of S is negative -- status 1, x and P held to the bar against the prediction, P exactly
    symmetric.  Every other family: status 0; P exactly symmetric there too."""
    ri = REGIMES.index(regime)
    for update in (True, False):
        idx, fam, args = _regime(fx, ri, update)
        out = _regime_outputs(ba, fx, ri, update)
        left = fam == fx["family_names"].index("prediction_left")
        assert len(idx) >= (12 if update else 2) and (not update or (left.sum() >= 2 and len(np.unique(fam)) == 5))
        assert np.array_equal(out[5], left.astype(np.int32)), out[5]
        assert np.array_equal(fx["status"][idx], out[5])
        assert np.array_equal(out[1], np.swapaxes(out[1], 1, 2)), "P is not exactly symmetric"
        assert np.array_equal(out[2], out[0][:, 19:22])
        _hold(f"1 {regime} {'update' if update else 'predict-only'} ticks (B = {len(idx)})", fx, ri, fam,
              _errors(out, fx["xn"][idx], from_triu(fx["Pnu"][idx]), fx["xw"][idx], fx["mp"][idx]))


@pytest.mark.parametrize("regime", REGIMES)
def test_rotated_batches_are_bit_identical(ba, fx, regime):
    """the same cases rotated by 1, 2 and 3 positions: every case sits in both halves of a wave, beside other neighbours"""
    ri = REGIMES.index(regime)
    par = _params(ba, fx["par"][ri])
    for update in (True, False):
        idx, fam, args = _regime(fx, ri, update)
        ref = _regime_outputs(ba, fx, ri, update)
        for s in (1, 2, 3):
            out = _tick(ba, par, *(np.roll(a, s, axis=0) for a in args), update=update)
            for a, b in zip(out, ref):
                assert np.array_equal(np.roll(a, -s, axis=0), b, equal_nan=True), (regime, update, s)


@pytest.mark.parametrize("regime", ["shipped", "varied"])
def test_one_filter_alone_and_a_tail_wave_with_one_live_filter(ba, fx, regime):
    """B = 1 (half of the wave idle) and B = 2 k + 1 (the last wave has one live filter): bit for bit what the full batch gives"""
    ri = REGIMES.index(regime)
    idx, fam, args = _regime(fx, ri, True)
    ref = _regime_outputs(ba, fx, ri, True)
    par = _params(ba, fx["par"][ri])
    n = FILTERS_PER_WAVE * ((len(idx) - 2) // FILTERS_PER_WAVE) + 1
    assert n % FILTERS_PER_WAVE == 1 and n >= 13
    out = _tick(ba, par, *(a[:n] for a in args))
    for a, b in zip(out, ref):
        assert np.array_equal(a, b[:n]), regime
    large = int(np.nonzero(fam == fx["family_names"].index("large_angle"))[0][1])      # the case with w < 0 in the quaternion product
    for c in (n - 1, large):
        out = _tick(ba, par, *(a[c:c + 1] for a in args))
        for a, b in zip(out, ref):
            assert np.array_equal(a, b[c:c + 1]), (regime, c)


# ---- 2. chains: the device carries its own state ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
def test_chain_of_six_ticks(ba, fx, regime):
    """3 filters x 6 ticks, predict-only and update ticks alternating: the reference carried its state at 60 digits, the numpy restatement its own
    in double (its error over all ticks is the family's E); the device carries its own and is held at EVERY tick"""
    ri = REGIMES.index(regime)
    fi = fx["family_names"].index("chain")
    K, B = fx["chain_xn"].shape[1:3]
    e = ba.BatchEskf(B, _params(ba, fx["par"][ri]))
    e.set_state(fx["chain_x0"][ri], from_triu(fx["P0u"][fx["chain_input"][ri]]))
    dev = []
    for k in range(K):
        if fx["chain_update"][ri, k]:
            e.update(*(fx["chain_" + n][ri, k] for n in ("imu", "gps_p", "gps_v", "qm", "thrust")))
        else:
            e.predict(fx["chain_imu"][ri, k])
        out = e.state() + e.outputs()
        assert not out[5].any(), (k, out[5])
        assert np.array_equal(out[1], np.swapaxes(out[1], 1, 2))
        dev.append(_errors(out, fx["chain_xn"][ri, k], from_triu(fx["chain_Pnu"][ri, k]), fx["chain_xw"][ri, k], fx["chain_mp"][ri, k]))
    e.close()
    dev = np.array(dev)         # [ticks, filters, quantities]
    _note(f"2 {regime} chain, worst x per tick", " ".join(f"{v:.2e}" for v in dev[:, :, 0].max(axis=1)))
    _hold(f"2 {regime} chain ({B} filters x {K} ticks)", fx, ri, np.full(K * B, fi), dev.reshape(K * B, 4))


# ---- 3. NaN inputs -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
def test_nan_inputs_are_flagged_and_stay_in_their_filter(ba, fx, regime):
    """a NaN in one filter's IMU sample reaches S through F: status 1, as the header states; a NaN in another's GPS position leaves S alone and
    makes the estimate not finite: status 2.  Every other filter of the batch, the wave neighbours of the two included: bit for bit what it
    is without them."""
    ri = REGIMES.index(regime)
    idx, fam, args = _regime(fx, ri, True)
    ref = _regime_outputs(ba, fx, ri, True)
    i_nan, g_nan = 0, 5                                       # wave 0, first half (its neighbour: filter 1); wave 2, second half (neighbour: 4)
    assert ref[5][i_nan] == 0 and ref[5][g_nan] == 0
    args = [a.copy() for a in args]
    args[2][i_nan, 4] = np.nan
    args[3][g_nan, 0] = np.nan
    out = _tick(ba, _params(ba, fx["par"][ri]), *args)
    others = np.ones(len(idx), dtype=bool); others[[i_nan, g_nan]] = False
    for a, b in zip(out, ref):
        assert np.array_equal(a[others], b[others]), regime
    st = out[5]
    _note(f"3 {regime} NaN inputs", f"IMU NaN: status {st[i_nan]}; GPS NaN: status {st[g_nan]}, x finite {bool(np.isfinite(out[0][g_nan]).all())}")
    assert st[i_nan] == 1 and st[g_nan] == 2 and not np.isfinite(out[0][g_nan]).all()
    assert np.isfinite(out[1][g_nan]).all()                   # the covariance does not see the measurement
