"""eskf_tick_masked_kernel (brov_imu_eskf_tick_host): one launch for a batch in which only some filters have a fix.  With fix[b] != 0 filter b does
exactly the update tick, with fix[b] == 0 exactly the predict-only tick: x, P, xi, xi_world, mpc_p and status bit for bit what the two existing
kernels give on the same batch.  States and inputs: the update ticks of the `loop` and `varied` regimes of tests/golden/eskf_exact.npz, which
this file only reads.  B in {1, 2, 3, 5}: a filter in the low half-wave, in the high half-wave, and beside a dead half-wave."""
import itertools
import os

import numpy as np
import pytest

from eskf_exact import from_triu, par_apply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIMES = ("shipped", "varied", "loop")
USED = ("loop", "varied")
NAMES = ("x", "P", "xi", "xi_world", "mpc_p", "status")
_REF = {}


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
    d["family_names"] = list(d["families"])
    assert tuple(d["regimes"]) == REGIMES
    return d


def _cases(fx, regime, B, first=0, family=None):
    """B update ticks of the regime from `first` on (or of one family): the parameters and (x, P, imu, gps_p, gps_v, q_meas, thrust)"""
    ri = REGIMES.index(regime)
    po = fx["family_names"].index("predict_only")
    sel = (fx["regime"] == ri) & (fx["family"] != po)
    if family is not None:
        sel &= fx["family"] == fx["family_names"].index(family)
    else:
        sel &= fx["status"] == 0
    idx = np.nonzero(sel)[0][first:first + B]
    assert len(idx) == B
    return fx["par"][ri], tuple(a.copy() for a in (fx["x0"][idx], from_triu(fx["P0u"][fx["input"][idx]]), fx["imu"][idx], fx["gps_p"][idx],
                                                    fx["gps_v"][idx], fx["qm"][idx], fx["thrust"][idx]))


def _tick(ba, par_vec, args, how):
    """how: 'update', 'predict', or the fix flags of the masked tick.  Returns x, P, xi, xi_world, mpc_p, status"""
    x, P, imu, gp, gv, qm, th = args
    e = ba.BatchEskf(len(x), par_apply(ba.EskfParams.default(), par_vec))
    e.set_state(x, P)
    if isinstance(how, str) and how == "update":
        e.update(imu, gp, gv, qm, th)
    elif isinstance(how, str):
        e.predict(imu)
    else:
        e.tick(imu, gp, gv, qm, th, np.asarray(how, dtype=np.int32))
    out = e.state() + e.outputs()
    e.close()
    return out


def _refs(ba, fx, regime, B):
    """the two existing kernels on the batch, computed once and left unchanged"""
    if (regime, B) not in _REF:
        par, args = _cases(fx, regime, B)
        _REF[regime, B] = (par, args, _tick(ba, par, args, "update"), _tick(ba, par, args, "predict"))
    return _REF[regime, B]


def _same(got, upd, pred, fix, what):
    """filter b of `got` is bit for bit filter b of the update batch where fix[b], of the predict-only batch where not"""
    for name, g, u, p in zip(NAMES, got, upd, pred):
        for b, f in enumerate(fix):
            want = u[b] if f else p[b]
            assert np.array_equal(g[b], want, equal_nan=True), (what, name, b, f)


@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("regime", USED)
def test_all_ones_is_update_and_all_zeros_is_predict(ba, fx, regime, B):
    par, args, upd, pred = _refs(ba, fx, regime, B)
    assert not upd[5].any() and not pred[5].any()
    assert not np.array_equal(upd[0], pred[0])                  # the two ticks differ: the comparison below tells them apart
    _same(_tick(ba, par, args, np.ones(B)), upd, pred, [1] * B, (regime, B, "ones"))
    _same(_tick(ba, par, args, np.zeros(B)), upd, pred, [0] * B, (regime, B, "zeros"))
    _same(_tick(ba, par, args, np.full(B, -7)), upd, pred, [1] * B, (regime, B, "any value but 0 is a fix"))


@pytest.mark.parametrize("regime", USED)
def test_every_mixed_pattern_of_three_filters(ba, fx, regime):
    """a full wave of two filters and a wave with a dead half: every pattern that is neither all ones nor all zeros"""
    par, args, upd, pred = _refs(ba, fx, regime, 3)
    for fix in itertools.product((0, 1), repeat=3):
        if sum(fix) in (0, 3):
            continue
        got = _tick(ba, par, args, fix)
        _same(got, upd, pred, fix, (regime, fix))
        assert np.array_equal(got[1], np.swapaxes(got[1], 1, 2)), "P is not exactly symmetric"


@pytest.mark.parametrize("regime", USED)
def test_nans_behind_a_missing_fix_reach_nothing(ba, fx, regime):
    """a filter without a fix whose gps_p, gps_v, q_meas and thrust are NaN: status 0 and the predict-only bits; its wave neighbour with a fix is
    what it is without them.  Both halves of the wave take the part of the filter without a fix."""
    par, args, upd, pred = _refs(ba, fx, regime, 2)
    for blind in (0, 1):
        a = [v.copy() for v in args]
        for j in (3, 4, 5, 6):
            a[j][blind] = np.nan
        fix = [1, 1]; fix[blind] = 0
        got = _tick(ba, par, a, fix)
        _same(got, upd, pred, fix, (regime, "blind", blind))
        assert got[5][blind] == 0 and all(np.isfinite(g[blind]).all() for g in got[:5])


@pytest.mark.parametrize("regime", USED)
def test_a_fix_on_a_covariance_whose_pivot_fails_still_reports_status_1(ba, fx, regime):
    """prediction_left: P = -(A A' + I / 2), the first pivot of S is negative.  With a fix: status 1, as the update tick reports; the same
    filter without a fix reports what the predict-only tick reports"""
    par, left = _cases(fx, regime, 1, family="prediction_left")
    _, other = _cases(fx, regime, 2)
    args = tuple(np.concatenate([o[:1], l, o[1:]]) for o, l in zip(other, left))      # the case in the high half of wave 0
    upd, pred = _tick(ba, par, args, "update"), _tick(ba, par, args, "predict")
    assert np.array_equal(upd[5], [0, 1, 0]) and pred[5][1] in (0, 2)
    for fix in ((1, 1, 1), (0, 1, 0), (1, 0, 1), (0, 1, 1)):
        got = _tick(ba, par, args, fix)
        _same(got, upd, pred, fix, (regime, "prediction_left", fix))
        assert got[5][1] == (1 if fix[1] else pred[5][1])
