"""GPU tests of the host-side foundation the four device objects share (csrc/host_common.hpp, solver._Handle): kernel timers, error
strings that stay per component, close() / destroy bookkeeping, and the one device-log struct of the closed loops.  Almost nothing is
launched; every refusal provoked here is a host-side argument check that returns before any device work."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
B, N = 3, 4


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


def _solver(ba, batch=B):
    s = ba.BatchSolver(batch, ba.SolverOptions(N, 0.05))
    s.set_params(ba.P_NOMINAL)
    return s


def _seconds_ok(t):
    assert np.isfinite(t) and t >= 0.0, t


def test_timers_refuse_before_the_first_update_and_report_after_it(ba):
    rng = np.random.default_rng(3)
    e, r, t = ba.BatchEkf(B), ba.BatchRls(B), ba.BatchTrack(B)
    for last in (e.last_update_seconds, r.last_update_seconds, t.last_seconds):
        with pytest.raises(RuntimeError):
            last()
    y12 = np.zeros((B, 12)); y12[:, 2] = -20.0
    e.update(rng.uniform(-2, 2, (B, 6)), y12, rng.uniform(-0.1, 0.1, (B, 6)))
    r.update(rng.uniform(-1, 1, (B, 4)), rng.uniform(-0.1, 0.1, (B, 4)), rng.uniform(-0.5, 0.5, (B, 4)), rng.uniform(-0.1, 0.1, (B, 3)))
    t.accumulate(rng.normal(size=(2, B, 12)), rng.uniform(-40, 40, (2, B, 4)), None, rng.normal(size=(4, 16)), 0)
    for last in (e.last_update_seconds, r.last_update_seconds, t.last_seconds):
        _seconds_ok(last())
    for o in (e, r, t):
        o.close()


def test_error_strings_stay_per_component(ba):
    s, e, e2, r = _solver(ba), ba.BatchEkf(B), ba.BatchEkf(2), ba.BatchRls(B)
    L = s._L
    ekf_before = L.brov_ekf_last_error()
    assert L.brov_solve_phase(s._h, C.c_void_p(0), 2) == -1          # feedback without a preparation
    with pytest.raises(RuntimeError):
        r.update_from_ekf(e2, s)                                     # an observer of another batch size
    assert b"brov_rls_update_from_ekf" in L.brov_rls_last_error()
    assert b"rti_phase" in L.brov_last_error()
    assert L.brov_ekf_last_error() == ekf_before
    for o in (s, e, e2, r):
        o.close()


def test_close_twice_is_harmless_and_destroy_returns_what_create_took(ba):
    first = _solver(ba)
    want = first.device_bytes
    assert want > 0
    first.close(); first.close()
    for make in (lambda: _solver(ba), lambda: ba.BatchEkf(B), lambda: ba.BatchRls(B), lambda: ba.BatchTrack(B)):
        for _ in range(2):
            o = make()
            o.close(); o.close()
            assert o._h is None
    fresh = _solver(ba)
    assert fresh.device_bytes == want
    fresh.close()


def test_closed_loop_ex_fills_logs_of_the_documented_shapes(ba):
    s = _solver(ba)
    x0 = np.zeros((B, 12)); x0[:, 2] = -20.0; x0[:, 0] = [0.0, 0.1, -0.1]
    s.set_x0(x0)
    traj = np.zeros((8, 16)); traj[:, 2] = -20.0
    s.set_trajectory(traj)
    ul, xl, sl, wl = s.closed_loop(2, line0=0, log_wrench=True)      # brov_closed_loop_ex
    assert ul.shape == (2, B, 4) and xl.shape == (3, B, 12) and sl.shape == (2, B) and wl.shape == (2, B, 6)
    assert sl.dtype == np.int32
    assert np.array_equal(xl[0], x0)
    assert np.array_equal(xl[2], s.get_x0())                          # ... and the last row is the state the loop left
    assert np.all(np.isfinite(ul)) and np.all(np.isfinite(xl)) and np.array_equal(wl, np.zeros_like(wl))
    s.close()
