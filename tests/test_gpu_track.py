"""GPU tests of the tracking statistics (brov_track_*, track_kernel.hip) and of the scored closed loop (brov_closed_loop_track) against
tests/track_restatement.py and against the logged loops on identically prepared twins.

Tolerances.  Integers and maxima are compared exactly.  Sums are compared at relative 1e-12 -- derived, not measured: a sum of n
non-negative terms differs between any two orders, with or without fused multiply-adds, by at most about n 2^-53 relative, below 1e-13
for every n here (at most 11 ticks per record, at most 3000 instance-ticks per summary)."""
import numpy as np
import pytest

from oracle import trajectory_oracle as T
from track_restatement import TrackRestatement

pytestmark = pytest.mark.gpu
SUMS = ("sum_pos2", "sum_yaw2", "sum_u2")
EXACT = ("max_pos2", "max_yaw", "ticks", "failed", "saturated", "nonfinite", "first_failed", "worst_tick", "pad_")
PERIODIC = dict(seed=0xC0FFEE123456789, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


def _same_stats(got, want, what=""):
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in SUMS:
        err = np.abs(got[k] - want[k]) / np.maximum(np.abs(want[k]), 1e-300)
        print(f"{what} {k}: worst relative difference {err.max():.2e}")
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=f"{what} {k}")


def _same_summary(got, want, what=""):
    for k in ("worst_max_pos2", "worst_instance", "ticks", "failed", "saturated", "nonfinite", "failed_instances"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("rms_pos", "rms_yaw"):
        print(f"{what} {k}: gpu {got[k]!r} restatement {want[k]!r}")
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=f"{what} {k}")
    assert got["worst_max_pos"] == float(np.sqrt(want["worst_max_pos2"]))


def _synthetic(B, K, seed, rows=12):
    """logs with planted cases: a NaN state in one instance-tick, an Inf input in another, statuses != 0, inputs exactly at lbu and at ubu;
    line1 is chosen so that the last two ticks lie past the table end"""
    rng = np.random.default_rng(seed)
    ref = rng.normal(size=(rows, 16)) * 3
    x = rng.normal(size=(K, B, 12)) * 2
    u = rng.uniform(-40, 40, (K, B, 4))
    st = np.zeros((K, B), dtype=np.int32)
    x[0, B // 2, 1] = np.nan
    u[K - 1, B // 4, 2] = np.inf
    st[0, B - 1] = 4; st[K - 1, B // 3] = 2; st[K - 1, B // 2] = 1
    u[0, min(1, B - 1), 0] = -50.0
    u[K - 1, B - 1, 3] = 50.0
    u[K // 2, (2 * B) // 3, 1] = np.nextafter(50.0, 0.0)      # just inside: not saturated
    return x, u, st, ref, rows - K + 2


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_accumulate_against_the_restatement(ba, B, K):
    x, u, st, ref, line1 = _synthetic(B, K, 100 * B + K)
    assert line1 + K - 2 > ref.shape[0] - 1
    t = ba.BatchTrack(B)
    t.accumulate(x, u, st, ref, line1)
    want = TrackRestatement(B).accumulate(x, u, st, ref, line1)
    _same_stats(t.stats(), want.stats(), f"B={B} K={K}")
    assert t.stats()["nonfinite"].sum() >= 1 and t.stats()["failed"].sum() >= 1
    if B >= 63:
        assert t.stats()["saturated"].sum() >= 2
    _same_summary(t.summary(), want.summary(), f"B={B} K={K}")
    if B == 65:
        # status = NULL counts as all zero; a negative line clamps to row 0; bounds of the tracker's own
        p = ba.TrackParams.default()
        for c in range(4):
            p.lbu[c], p.ubu[c] = -30.0 - c, 20.0 + c
        t2 = ba.BatchTrack(B, p)
        t2.accumulate(x, u, None, ref, -2)
        want2 = TrackRestatement(B, [-30, -31, -32, -33], [20, 21, 22, 23]).accumulate(x, u, None, ref, -2)
        _same_stats(t2.stats(), want2.stats(), "no status")
        assert not t2.stats()["failed"].any() and t2.stats()["saturated"].sum() > want.stats()["saturated"].sum()
        assert t2.last_seconds() > 0.0
        t2.close()
    # reset: back to the empty record
    t.reset()
    assert t.stats().tobytes() == TrackRestatement(B).stats().tobytes()
    t.close()


def test_the_record_does_not_depend_on_how_a_run_is_cut(ba):
    B, K = 65, 7
    x, u, st, ref, _ = _synthetic(B, K, 7)
    line1 = 8                                         # 12 rows: ticks 4 .. 6 clamp
    out = []
    for cuts in ([7], [3, 4], [1] * 7):
        t = ba.BatchTrack(B)
        k = 0
        for n in cuts:
            t.accumulate(x[k:k + n], u[k:k + n], st[k:k + n], ref, line1 + k)
            k += n
        out.append(t.stats())
        t.close()
    assert out[0].tobytes() == out[1].tobytes() == out[2].tobytes()
    _same_stats(out[0], TrackRestatement(B).accumulate(x, u, st, ref, line1).stats(), "7 ticks")


@pytest.mark.parametrize("B", [257, 1000])
def test_summary_against_the_restatement(ba, B):
    K = 3
    x, u, st, ref, _ = _synthetic(B, K, 11 + B)
    line1 = 2
    x[:, 5] = np.nan                                  # an instance without a counted tick, with a failed tick
    st[1, 5] = 3
    hi, lo = (B * 9) // 10, B // 5                    # a tie for the worst instance, the higher index in another block
    x[1, hi] = x[1, lo] = ref[line1 + 1, :12] + 100.0
    u[1, hi] = u[1, lo]
    t = ba.BatchTrack(B)
    t.accumulate(x, u, st, ref, line1)
    want = TrackRestatement(B).accumulate(x, u, st, ref, line1)
    _same_stats(t.stats(), want.stats(), f"B={B}")
    ws = want.summary()
    assert ws["worst_instance"] == lo and want.stats()["max_pos2"][hi] == ws["worst_max_pos2"] and want.stats()["ticks"][5] == 0
    _same_summary(t.summary(), ws, f"B={B}")
    assert t.summary_bytes() == t.summary_bytes()
    # no counted tick at all
    t.reset()
    s = t.summary()
    assert (s["rms_pos"], s["rms_yaw"], s["worst_max_pos2"], s["worst_instance"], s["ticks"], s["failed_instances"]) == (0.0, 0.0, 0.0, -1, 0, 0)
    t.close()


def _start(ba, B, seed):
    rng = np.random.default_rng(seed)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
    x0[B - 1, :3] += [4.0, -4.0, 3.0]                 # one instance metres off: its inputs sit on the bounds
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = rng.uniform(-30, 30, (B, 4))
    return traj, x0, pp


def _solver(ba, B, N, x0, traj, pp, wrench=None):
    s = ba.BatchSolver(B, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(pp); s.set_trajectory(traj)
    if wrench is not None:
        s.set_plant_wrench(**wrench)
    return s


@pytest.mark.parametrize("N,chunk,wrench", [(10, 0, False), (10, 3, False), (10, 7, False), (24, 0, False), (24, 3, False), (24, 7, False),
                                            (10, 3, True)])
def test_tracked_loop_equals_the_logged_loop(ba, N, chunk, wrench):
    B, ticks, more, line0 = 5, 7, 4, 2
    traj, x0, pp = _start(ba, B, 31)
    w = dict(constant=[10, 10, 10, 0, 0, 0]) if wrench else None
    a, b = _solver(ba, B, N, x0, traj, pp, w), _solver(ba, B, N, x0, traj, pp, w)
    t = ba.BatchTrack(B)
    want = TrackRestatement(B)
    a.closed_loop_track(t, ticks, line0=line0, chunk=chunk)
    ul, xl, sl = b.closed_loop(ticks, line0=line0)
    assert a.get_x0().tobytes() == b.get_x0().tobytes() and a.results().tobytes() == b.results().tobytes()
    assert a.last_kernel_path() == b.last_kernel_path() and a.plant_wrench_tick() == b.plant_wrench_tick() == ticks
    want.accumulate(xl[1:], ul, sl, traj, line0 + 1)
    _same_stats(t.stats(), want.stats(), f"N={N} chunk={chunk} wrench={wrench}")
    # (every tick is either counted or non-finite: the instance that starts metres off may diverge, full-step SQP has no globalisation)
    assert (t.stats()["ticks"] + t.stats()["nonfinite"] == ticks).all() and (t.stats()["ticks"][:B - 1] == ticks).all()
    print("saturated ticks per instance:", t.stats()["saturated"], "non-finite:", t.stats()["nonfinite"])
    # a second call continues the record
    a.closed_loop_track(t, more, line0=line0 + ticks, chunk=chunk)
    ul, xl, sl = b.closed_loop(more, line0=line0 + ticks)
    assert a.get_x0().tobytes() == b.get_x0().tobytes() and a.results().tobytes() == b.results().tobytes()
    want.accumulate(xl[1:], ul, sl, traj, line0 + ticks + 1)
    _same_stats(t.stats(), want.stats(), f"N={N} chunk={chunk} wrench={wrench}, 11 ticks")
    assert (t.stats()["ticks"] + t.stats()["nonfinite"] == ticks + more).all() and (t.stats()["ticks"][:B - 1] == ticks + more).all()
    _same_summary(t.summary(), want.summary(), "loop")
    a.close(); b.close(); t.close()


def _observer(ba, B, with_rls):
    """observer (and estimator) for the device plant: unit scaling, no roll / pitch thrust (tests/test_gpu_plant_wrench.py, _ekf_pair)"""
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
    r = None
    if with_rls:
        rp = ba.RlsParams.default(); rp.compensate_coef = 1.0; rp.rotor_constant = 1.0
        r = ba.BatchRls(B, rp)
    return ba.BatchEkf(B, par), r


@pytest.mark.parametrize("with_rls", [False, True])
def test_tracked_loop_with_the_observer_equals_the_logged_dob_loop(ba, with_rls):
    B, N, ticks, chunk, line0 = 4, 10, 6, 4, 1
    traj, x0, pp = _start(ba, B, 41)
    a, b = _solver(ba, B, N, x0, traj, pp, dict(periodic=PERIODIC)), _solver(ba, B, N, x0, traj, pp, dict(periodic=PERIODIC))
    (ea, ra), (eb, rb) = _observer(ba, B, with_rls), _observer(ba, B, with_rls)
    t = ba.BatchTrack(B)
    a.closed_loop_track(t, ticks, line0=line0, ekf=ea, rls=ra, rls_mode=ba.APPLY_DISTURBANCE, chunk=chunk)
    log = b.closed_loop_dob(eb, rb, ba.APPLY_DISTURBANCE, ticks=ticks, line0=line0)
    assert a.get_x0().tobytes() == b.get_x0().tobytes() and a.results().tobytes() == b.results().tobytes()
    assert a.get_params().tobytes() == b.get_params().tobytes() and a.plant_wrench_tick() == b.plant_wrench_tick() == ticks
    for p, q in zip(ea.state(), eb.state()):
        assert p.tobytes() == q.tobytes()
    if with_rls:
        for p, q in zip(ra.state(), rb.state()):
            assert p.tobytes() == q.tobytes()
    assert a.get_params()[:, :, :4].any()                       # the hand-off reached the controller
    want = TrackRestatement(B).accumulate(log["x"][1:], log["u"], log["status"], traj, line0 + 1)
    _same_stats(t.stats(), want.stats(), f"observer, rls={with_rls}")
    assert (t.stats()["ticks"] + t.stats()["nonfinite"] == ticks).all() and (t.stats()["ticks"][:B - 1] == ticks).all()
    for o in (a, b, ea, eb, t) + ((ra, rb) if with_rls else ()):
        o.close()


def test_refusals_leave_the_record_alone(ba):
    B, N = 4, 10
    traj, x0, pp = _start(ba, B, 51)
    s = _solver(ba, B, N, x0, traj, pp)
    t, other = ba.BatchTrack(B), ba.BatchTrack(B + 1)
    s.closed_loop_track(t, 2)
    before, x_before = t.stats().tobytes(), s.get_x0().tobytes()
    bare = ba.BatchSolver(B, ba.SolverOptions(N))                      # no trajectory table
    e, _ = _observer(ba, B + 1, False)
    for call in (lambda: s.closed_loop_track(other, 2), lambda: s.closed_loop_track(t, 0), lambda: s.closed_loop_track(t, 2, chunk=-1),
                 lambda: bare.closed_loop_track(t, 2), lambda: s.closed_loop_track(t, 2, ekf=e)):
        with pytest.raises(RuntimeError, match=r"closed_loop_track failed \(-1\)"):
            call()
        assert t.stats().tobytes() == before and s.get_x0().tobytes() == x_before
    assert not other.stats()["ticks"].any()
    for o in (s, bare, t, other, e):
        o.close()
