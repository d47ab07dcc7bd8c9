"""GPU tests of the fleet planning loop (brov_fleet_*, brov_closed_loop_fleet; bluerov2_amd/csrc/fleet_kernel.hip): the segmented select
against the numpy restatement byte for byte, the closed loop against loops composed from the calls that existed before it, the hold /
status rule, and the argument checks.  N = 20 throughout, at most 650 instances."""
import ctypes

import numpy as np
import pytest

import fleet_restatement as FR

pytestmark = pytest.mark.gpu
N, TS = 20, 0.05
X_TOL = 1e-12          # what tests/test_gpu_closed_loop.py holds the plant step to against orc_rk4
ERR_ARG = -1


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


def solver(ba, B):
    s = ba.BatchSolver(B, ba.SolverOptions(N, TS))
    s.set_params(ba.P_NOMINAL)
    return s


def synthetic_records(V, C, seed):
    """records with costs of mixed sign from a fixed seed, every field filled, a sprinkling of failed candidates"""
    rng = np.random.default_rng(seed)
    B = V * C
    r = np.zeros(B, dtype=FR.RESULT_DTYPE)
    r["u0"] = rng.uniform(-20, 20, (B, 4)); r["cost"] = rng.normal(size=B) * 10; r["kkt"] = rng.uniform(0, 5, B)
    r["qp_iter"] = rng.integers(0, 9, B); r["thrust"] = rng.normal(size=(B, 6))
    r["status"] = np.where(rng.uniform(size=B) < 0.2, rng.integers(1, 5, B), 0)
    return r


def check_select(f, r, V, C):
    w, wr = f.select(r)
    ew, ewr = FR.select(r, V, C)
    assert np.array_equal(w, ew), (V, C, w, ew)
    assert wr.tobytes() == ewr.tobytes()
    w2, wr2 = f.select(r)
    assert w2.tobytes() == w.tobytes() and wr2.tobytes() == wr.tobytes()     # two calls, the same bytes
    w3, none = f.select(r, with_records=False)
    assert none is None and np.array_equal(w3, ew)
    return ew


@pytest.mark.parametrize("V,C", [(1, 1), (5, 3), (3, 64), (2, 65), (2, 130), (1, 650)])
def test_select_equals_the_restatement_byte_for_byte(ba, V, C):
    s = solver(ba, V * C)
    f = ba.Fleet(s, C)
    assert (f.V, f.C) == (V, C)
    r = synthetic_records(V, C, seed=100 * V + C)
    check_select(f, r, V, C)
    # every cost equal within a group: index 0
    q = r.copy(); q["status"] = 0; q["cost"] = np.repeat(np.arange(V) - 0.5, C)
    assert not check_select(f, q, V, C).any()
    # the only eligible candidate is the last one of every group: the last lane of the last pass
    q = r.copy(); q["status"] = 4; q["status"][C - 1::C] = 0; q["cost"][C - 1::C] = 3.0
    assert list(check_select(f, q, V, C)) == [C - 1] * V
    # a group with no eligible candidate beside groups that have one
    q = r.copy(); q["status"] = 0; q["status"][:C] = 2
    w = check_select(f, q, V, C)
    assert w[0] == -1 and np.all(w[1:] >= 0)
    # +-Inf and NaN costs with status 0 never win; where nothing else is left the group has no winner
    q = r.copy(); q["status"] = 0
    q["cost"][0::3] = np.nan; q["cost"][1::3] = -np.inf; q["cost"][2::3] = np.inf
    assert np.all(check_select(f, q, V, C) == -1)
    if C >= 3:
        q["cost"][C // 2::C] = 7.0
        assert list(check_select(f, q, V, C)) == [C // 2] * V
    # the lowest cost carried by a failed candidate
    q = r.copy(); q["status"] = 0; q["cost"] = np.abs(q["cost"]) + 1.0
    q["cost"][C - 1::C] = -1e9; q["status"][C - 1::C] = 3
    w = check_select(f, q, V, C)
    assert np.all(w != C - 1)
    f.close(); s.close()


def test_select_of_one_group_equals_select_best_on_a_real_solve(ba):
    B = 130
    rng = np.random.default_rng(4)
    s = solver(ba, B)
    x0 = np.zeros((B, 12)); x0[:, 0] = -2.0; x0[:, 2] = -20.0; x0[:, 5] = -0.5 * np.pi
    s.set_x0(x0)
    s.set_candidate_params("circle", rng.uniform(1.5, 3.0, B), rng.uniform(0.2, 0.8, B), np.zeros(B))
    for k in range(2):
        s.set_yref_candidates_tick(TS * k, TS); s.solve()
    r = s.results()
    assert np.all(np.isfinite(r["cost"])) and np.all(r["cost"] < 1e300) and (r["status"] == 0).any()
    f = ba.Fleet(s, B)
    w, wr = f.select()                      # the solver's own records
    idx, rec = s.select_best()
    assert w[0] == idx == FR.select(r, 1, B)[0][0]
    assert wr[0].tobytes() == rec.tobytes() == r[idx].tobytes()
    assert f.last_seconds() > 0.0
    f.close(); s.close()


def test_one_candidate_per_vehicle_is_the_existing_loop(ba):
    B, ticks = 8, 6
    rng = np.random.default_rng(7)
    amp, frq, ph = rng.uniform(1, 3, B), rng.uniform(0.25, 0.75, B), rng.uniform(0, 2 * np.pi, B)
    x0 = np.zeros((B, 12)); x0[:, 0] = amp * np.cos(ph); x0[:, 1] = amp * np.sin(ph) * np.cos(ph); x0[:, 2] = -20.0
    x0 += rng.normal(size=(B, 12)) * 0.02
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = rng.uniform(-5, 5, (B, 4))
    t0, dt_ref = 0.3, 0.05
    a, b = solver(ba, B), solver(ba, B)
    for s in (a, b):
        s.set_x0(x0); s.set_candidate_params("lemniscate", amp, frq, ph)
    f = ba.Fleet(a, 1)                      # (create takes the vehicles' states from the solver's x0)
    f.set_plant_params(pp); b.set_plant_params(pp)
    ul, xl, sl, wl = f.closed_loop(ticks, t0=t0, dt_ref=dt_ref, dt_node=TS, dt=0.05, substeps=2)
    assert np.array_equal(xl[0], x0)
    ur, xr, sr = np.empty_like(ul), np.empty_like(xl), np.empty_like(sl)
    xr[0] = x0
    for k in range(ticks):
        b.set_yref_candidates_tick(t0 + k * dt_ref, TS); b.solve()
        res = b.results()
        b.plant_step(0.05, 2)
        ur[k], sr[k], xr[k + 1] = res["u0"], res["status"], b.get_x0()
    assert np.array_equal(sl, sr) and np.array_equal(ul, ur)
    assert np.array_equal(wl, np.where(sr == 0, 0, -1))
    err = np.abs(xl - xr).max()
    print(f"[fleet C=1] max |x_fleet - x_plant_step| = {err:.3e}, bit-identical: {xl.tobytes() == xr.tobytes()}")
    assert err <= X_TOL
    assert np.array_equal(f.state(), xl[-1]) and np.array_equal(a.get_x0(), xl[-1])
    f.close(); a.close(); b.close()


def test_three_loops_step_one_plant(ba):
    """The same closed loop three ways from the same start: brov_closed_loop in one launch (the plant inside the *_ticks kernel),
    brov_closed_loop as three launches per tick (plant_kernel) and the fleet loop with one candidate per vehicle (fleet_plant_kernel).  The
    first two log the same bytes.  The fleet's plant is the same plant_inputs / plant_erk4 call as plant_kernel's, compiled into another
    kernel; on the MI355X it logs the same bytes as well (profiles/plant_step_refactor_isa.txt, section 5), and that is asserted.
        Ts = 1/16, a power of two: the node times (k + i) Ts of the table rows and k Ts + i Ts of the
    fleet's windows are then the same doubles, and the table is cut from the device's own generator."""
    import os
    B, ticks, Ts = 8, 3, 0.0625
    rng = np.random.default_rng(21)
    amp, frq, ph = np.full(B, 2.0), np.full(B, 0.5), np.full(B, 0.4)          # one shape: the table of brov_closed_loop is shared
    x0 = np.zeros((B, 12)); x0[:, 0] = 2.0 * np.cos(0.4); x0[:, 1] = 2.0 * np.sin(0.4) * np.cos(0.4); x0[:, 2] = -20.0
    x0 += rng.normal(size=(B, 12)) * 0.02
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = rng.uniform(-5, 5, (B, 4)); pp[:, 4:] *= rng.uniform(0.9, 1.1, (B, 12))
    logs = []
    for fused in ("1", "0"):
        os.environ["BROV_CLOSED_LOOP_FUSED"] = fused
        try:
            s = ba.BatchSolver(B, ba.SolverOptions(N, Ts))
        finally:
            os.environ.pop("BROV_CLOSED_LOOP_FUSED", None)
        s.set_params(ba.P_NOMINAL); s.set_plant_params(pp)
        s.set_yref_candidates("lemniscate", amp, frq, ph, t0=0.0, dt=Ts); head = s.get_yref()[0]
        s.set_yref_candidates("lemniscate", amp, frq, ph, t0=ticks * Ts, dt=Ts); tail = s.get_yref()[0]
        assert np.array_equal(head[ticks:], tail[:N + 1 - ticks])             # the rows are functions of the node time alone
        s.set_trajectory(np.vstack([head, tail[N + 1 - ticks:]]))
        s.set_x0(x0)
        logs.append(s.closed_loop(ticks, line0=0, ncols=16, dt=0.05, substeps=2))
        s.close()
    (u1, x1, s1), (u0, x0l, s0) = logs
    assert not s1.any() and np.array_equal(s1, s0)
    assert u1.tobytes() == u0.tobytes() and x1.tobytes() == x0l.tobytes()
    a = ba.BatchSolver(B, ba.SolverOptions(N, Ts))
    a.set_params(ba.P_NOMINAL); a.set_x0(x0); a.set_candidate_params("lemniscate", amp, frq, ph)
    f = ba.Fleet(a, 1)
    f.set_plant_params(pp)
    uf, xf, sf, wf = f.closed_loop(ticks, t0=0.0, dt_ref=Ts, dt_node=Ts, dt=0.05, substeps=2)
    f.close(); a.close()
    assert not sf.any() and not wf.any()
    err = np.abs(xf - x1).max()
    print(f"[three loops] fleet against brov_closed_loop: u bit-identical: {uf.tobytes() == u1.tobytes()}, max |dx| = {err:.3e}, "
          f"x bit-identical: {xf.tobytes() == x1.tobytes()}")
    assert uf.tobytes() == u1.tobytes() and xf.tobytes() == x1.tobytes()


@pytest.mark.parametrize("V,C", [(5, 3), (2, 65)])
def test_closed_loop_against_a_loop_composed_on_the_host(ba, V, C):
    B, ticks = V * C, 4
    rng = np.random.default_rng(10 * V + C)
    radius = np.tile(2.0 + 0.5 * np.arange(C) / C, V)              # distinct radii per candidate
    speed, phase = np.full(B, 0.5), np.zeros(B)
    xv = np.zeros((V, 12)); xv[:, 0] = -2.2; xv[:, 2] = -20.0; xv[:, 5] = -0.5 * np.pi
    xv[:, :3] += rng.normal(size=(V, 3)) * 0.1                      # distinct start states per vehicle
    xv[:, 5] += rng.normal(size=V) * 0.05
    a, b = solver(ba, B), solver(ba, B)
    for s in (a, b):
        s.set_candidate_params("circle", radius, speed, phase)
    f = ba.Fleet(a, C)
    f.set_state(xv)
    assert np.array_equal(a.get_x0(), np.repeat(xv, C, axis=0))
    b.set_x0(np.repeat(xv, C, axis=0))
    ul, xl, sl, wl = f.closed_loop(ticks, t0=0.0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1)
    ur, xr, sr, wr = np.empty_like(ul), np.empty_like(xl), np.empty_like(sl), np.empty_like(wl)
    xr[0] = xv
    hold = np.zeros((V, 4))
    for k in range(ticks):
        b.set_yref_candidates_tick(0.0 + k * TS, TS); b.solve()
        res = b.results()
        wr[k], ur[k], sr[k] = FR.apply(res, V, C, hold)
        assert np.all(wr[k] >= 0), "the composed loop cannot hold an input: every vehicle needs a winner"
        hold = ur[k]
        b.plant_step(0.05, 1)                                       # every candidate with its own u0 ...
        xr[k + 1] = b.get_x0()[np.arange(V) * C + wr[k]]            # ... the winner's is the vehicle's
        b.set_x0(np.repeat(xr[k + 1], C, axis=0))
    assert np.array_equal(wl, wr), (wl, wr)
    assert np.array_equal(sl, sr) and np.array_equal(ul, ur)
    err = np.abs(xl - xr).max()
    print(f"[fleet V={V} C={C}] max |x_fleet - x_composed| = {err:.3e}, bit-identical: {xl.tobytes() == xr.tobytes()}, winners {wl.tolist()}")
    assert err <= X_TOL
    assert len(set(wl.ravel().tolist())) > 1                        # the run does choose between candidates
    # every candidate's x0 is its vehicle's state, bit for bit
    assert a.get_x0().tobytes() == np.repeat(f.state(), C, axis=0).tobytes() and np.array_equal(f.state(), xl[-1])
    f.close(); a.close(); b.close()


def _device_records(r):
    import torch
    return torch.from_numpy(np.frombuffer(r.tobytes(), dtype=np.uint8).copy()).cuda()


def test_hold_status_and_reset(ba):
    V = C = 3
    rng = np.random.default_rng(12)
    xv = np.zeros((V, 12)); xv[:, 2] = -20.0; xv[:, :2] = rng.normal(size=(V, 2))
    r1 = synthetic_records(V, C, seed=1); r1["status"] = 0
    r2 = synthetic_records(V, C, seed=2); r2["status"] = 0
    r2f = r2.copy(); r2f["status"][C:2 * C] = [4, 2, 3]             # vehicle 1: every candidate failed
    runs = {}
    for name, second in (("fail", r2f), ("ok", r2)):
        s = solver(ba, V * C)
        f = ba.Fleet(s, C)
        f.set_state(xv)
        d1, d2 = _device_records(r1), _device_records(second)
        f.step(d1.data_ptr(), 0.05, 1)
        u1, st1, w1 = f.last()
        ew, eu, es = FR.apply(r1, V, C, np.zeros((V, 4)))
        assert np.array_equal(w1, ew) and np.array_equal(u1, eu) and not st1.any()
        f.step(d2.data_ptr(), 0.05, 1)
        u2, st2, w2 = f.last()
        ew, eu, es = FR.apply(second, V, C, u1)
        assert np.array_equal(w2, ew) and np.array_equal(u2, eu) and np.array_equal(st2, es)
        runs[name] = (u1, u2, st2, w2, f.state(), s.get_x0())
        if name == "fail":
            assert w2[1] == -1 and st2[1] == 4 and np.array_equal(u2[1], u1[1])     # held input, candidate 0's status
            # after a reset the held input is zero
            f.reset()
            f.step(d2.data_ptr(), 0.05, 1)
            u3, st3, w3 = f.last()
            assert not u3[1].any() and w3[1] == -1 and st3[1] == 4
            # success with a NaN cost on candidate 0 (and nobody eligible): STATUS_NAN
            rn = r2.copy(); rn["cost"][C:2 * C] = [np.nan, np.inf, -np.inf]
            dn = _device_records(rn)
            f.step(dn.data_ptr(), 0.05, 1)
            u4, st4, w4 = f.last()
            assert w4[1] == -1 and st4[1] == FR.STATUS_NAN and not u4[1].any() and st4[0] == 0 and st4[2] == 0
            ba_torch_sync()
        f.close(); s.close()
    # vehicles 0 and 2 do not see vehicle 1's failure
    for v in (0, 2):
        assert runs["fail"][4][v].tobytes() == runs["ok"][4][v].tobytes()
        assert runs["fail"][5][v * C:(v + 1) * C].tobytes() == runs["ok"][5][v * C:(v + 1) * C].tobytes()
        assert np.array_equal(runs["fail"][1][v], runs["ok"][1][v])
    assert runs["fail"][4][1].tobytes() != runs["ok"][4][1].tobytes()


def ba_torch_sync():
    import torch
    torch.cuda.synchronize()


def test_arguments(ba):
    from bluerov2_amd.fleet import _fleet_lib
    L = _fleet_lib()
    B, C = 6, 3
    s = solver(ba, B)
    x0 = np.arange(B * 12, dtype=np.float64).reshape(B, 12) * 0.01; x0[:, 2] = -20.0
    s.set_x0(x0)

    def refused(rc):
        assert rc == ERR_ARG and L.brov_fleet_last_error().decode()
        assert np.array_equal(s.get_x0(), x0)

    h = ctypes.c_void_p()
    refused(L.brov_fleet_create(ctypes.byref(h), s._h, 4))          # B % C != 0
    assert not h.value
    refused(L.brov_fleet_create(ctypes.byref(h), s._h, 0))
    refused(L.brov_fleet_create(ctypes.byref(h), s._h, B + 1))
    with pytest.raises(RuntimeError):
        ba.Fleet(s, 4)
    f = ba.Fleet(s, C)
    loop = lambda ticks, *logs: L.brov_closed_loop_fleet(f._h, ticks, 0.0, TS, TS, 0.05, 1, *logs)   # noqa: E731
    none = (None, None, None, None)
    refused(loop(2, *none))                                         # no candidate parameters uploaded
    s.set_candidate_params("circle", np.full(B, 2.0), np.full(B, 0.5), np.zeros(B))
    # log arrays of a failing call are untouched
    u = np.full((2, 2, 4), 7.0); x = np.full((3, 2, 12), 7.0); st = np.full((2, 2), 7, dtype=np.int32); win = np.full((2, 2), 7, dtype=np.int32)
    logs = (u.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), win.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    refused(loop(-1, *logs))                                        # ticks < 0
    refused(L.brov_closed_loop_fleet(f._h, 2, 0.0, TS, TS, 0.0, 1, *logs))
    refused(L.brov_closed_loop_fleet(f._h, 2, 0.0, TS, TS, 0.05, 0, *logs))
    s.set_plant_wrench(constant=[10, 10, 10, 0, 0, 0])              # a wrench mode in force
    refused(loop(2, *logs))
    refused(L.brov_fleet_step(f._h, None, 0.05, 1, None))
    s.plant_wrench_off()
    s.enable_dist6(True)                                            # the 6-disturbance variant on
    refused(loop(2, *logs))
    refused(L.brov_fleet_step(f._h, None, 0.05, 1, None))
    s.enable_dist6(False)
    assert np.all(u == 7.0) and np.all(x == 7.0) and np.all(st == 7) and np.all(win == 7)
    # ... and with the modes off again the same call runs
    assert loop(2, *logs) == 0
    assert np.array_equal(x[0], x0[::C]) and not np.any(x == 7.0) and not np.any(u == 7.0) and np.all(win >= -1) and np.all(win < C)
    f.close(); s.close()
