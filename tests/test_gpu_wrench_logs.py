"""GPU tests of the two pieces of host code the solver and the fleet share: the wrench source behind
brov_plant_wrench_* and brov_vehicle_wrench_* (bluerov2_amd/csrc/wrench_source.hpp) and the loop log behind brov_closed_loop_ex / _dob /
_track and the fleet's loops (LoopLog, host_common.hpp).  Both owners get the same refusals, the same edge of the periodic range and the
same "any subset of logs" contract; the solver's wrench buffers appear in brov_device_bytes() once, on first use.  Tiny shapes: a solver of
B = 3 at N = 10 over a table of 3 + N + 2 rows, a fleet of 2 vehicles x 3 candidates, 3 ticks."""
import ctypes
import math

import numpy as np
import pytest

from oracle import trajectory_oracle as T
from track_restatement import TrackRestatement

pytestmark = pytest.mark.gpu
B, N, TICKS, LINE0 = 3, 10, 3, 1
V, C = 2, 3
TS = 0.05
OK, ERR_ARG = 0, -1
PERIODIC = dict(seed=0xC0FFEE123456789, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)
EDGE = int(2 ** 22 * math.pi)                 # the last tick whose half-period index has 22 bits under dphi = 1
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


def dp(a):
    return None if a is None else a.ctypes.data_as(DP)


def ip(a):
    return None if a is None else a.ctypes.data_as(IP)


def _traj():
    return np.ascontiguousarray(T.circle()[:3 + N + 2])


def _solver(ba, batch=B, seed=4):
    """a solver on the short table, distinct start states and plant parameters; returns (solver, x0)"""
    rng = np.random.default_rng(seed)
    traj = _traj()
    x0 = np.zeros((batch, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(batch, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
    pp = np.tile(ba.P_NOMINAL, (batch, 1)); pp[:, :4] = rng.uniform(-30, 30, (batch, 4))
    s = ba.BatchSolver(batch, ba.SolverOptions(N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(pp); s.set_trajectory(traj)
    return s, x0


def _fleet(ba, vehicles=V, cands=C, seed=6):
    """a fleet over circle candidates of distinct radii, distinct start states and true parameters; returns (solver, fleet, xv)"""
    n = vehicles * cands
    rng = np.random.default_rng(seed)
    s = ba.BatchSolver(n, ba.SolverOptions(N, TS))
    s.set_params(ba.P_NOMINAL)
    s.set_candidate_params("circle", np.tile(2.0 + 0.5 * np.arange(cands) / cands, vehicles), np.full(n, 0.5), np.zeros(n))
    xv = np.zeros((vehicles, 12)); xv[:, 0] = -2.2; xv[:, 2] = -20.0; xv[:, 5] = -0.5 * np.pi
    xv[:, :3] += rng.normal(size=(vehicles, 3)) * 0.1
    pp = np.tile(ba.P_NOMINAL, (vehicles, 1)); pp[:, :4] = rng.uniform(-5, 5, (vehicles, 4))
    f = ba.Fleet(s, cands)
    f.set_state(xv); f.set_plant_params(pp)
    return s, f, xv


def _ekf(ba, batch):
    """the observer for the device plant: unit scaling, no roll / pitch thrust (the helper of tests/test_gpu_plant_wrench.py restated)"""
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
    return ba.BatchEkf(batch, par)


class _Owner:
    """one owner of a wrench source through raw ctypes: the solver (brov_plant_wrench_*) or the fleet (brov_vehicle_wrench_*)"""

    def __init__(self, L, prefix, handle, last_error, poison):
        self.L, self.prefix, self.h, self._last_error, self._poison = L, prefix, handle, last_error, poison

    def fn(self, op):
        return getattr(self.L, self.prefix + op)

    def text(self):
        return getattr(self.L, self._last_error)().decode()

    def poison(self):
        """a refusal of an unrelated entry point of the same component: its text is what an entry point that writes none leaves behind"""
        assert self._poison() == ERR_ARG
        return self.text()

    def state(self, batch):
        w = np.full((batch, 6), 7.0)
        assert self.fn("eval_host")(self.h, 3, dp(w)) == OK
        return int(self.fn("mode")(self.h)), int(self.fn("tick")(self.h)), w.tobytes()


def _owners(ba, s, f):
    from bluerov2_amd.fleet import _fleet_lib
    from bluerov2_amd.solver import _load
    L = _load(); _fleet_lib()
    return [_Owner(L, "brov_plant_wrench_", s._h, "brov_last_error", lambda: L.brov_create(None, 0, 1, None)),
            _Owner(L, "brov_vehicle_wrench_", f._h, "brov_fleet_last_error", lambda: L.brov_fleet_create(None, None, 1))]


# ---- 1. one refusal table, two owners ---------------------------------------------------------------------------------------------------
def test_one_refusal_table_two_owners(ba):
    s, _ = _solver(ba, V)
    sf = ba.BatchSolver(V, ba.SolverOptions(N, TS))
    f = ba.Fleet(sf, 1)
    owners = _owners(ba, s, f)
    wc = np.arange(V * 6, dtype=np.float64).reshape(V, 6) + 1.0
    buf = np.full((V, 6), 7.0)
    inf, nan = float("inf"), float("nan")
    # (entry point, arguments behind the handle)
    null_handle = [("constant_host", (dp(wc),)), ("periodic", (1, 6.0, 0.0, 0.125, 3.0)), ("table_host", (dp(wc), V, None)), ("off", ()),
                   ("seek", (3,)), ("eval_host", (3, dp(buf)))]
    under_constant = [("constant_host", (None,)), ("eval_host", (3, None)), ("table_host", (None, 2, None)), ("table_host", (dp(wc), 0, None)),
                      ("periodic", (1, 6.0, 0.0, 0.125, 0.0)), ("periodic", (1, inf, 0.0, 0.125, 3.0)), ("periodic", (1, nan, 0.0, 0.125, 3.0)),
                      ("periodic", (1, 6.0, -1.0, 0.125, 3.0)), ("seek", (-1,))]
    under_dphi_1 = [("seek", (EDGE + 8,)), ("eval_host", (EDGE + 8, dp(buf)))]
    at_the_edge = [("periodic", (1, 6.0, 8.0, 1.0, 3.0))]       # phase0 = 8: tick EDGE, where the counter stands, is out of range
    no_text = []

    def refuse(o, other, batch, op, args, handle):
        before = o.state(batch)
        mine, theirs = o.poison(), other.poison()
        rc = o.fn(op)(handle, *args)
        assert rc == ERR_ARG, (o.prefix + op, args, rc)
        assert other.text() == theirs, (o.prefix + op, "wrote the other owner's error string")
        if o.text() == mine or not o.text().startswith(o.prefix + op):
            no_text.append((o.prefix + op, "null handle" if handle is None else args, o.text()))
        assert o.state(batch) == before, (o.prefix + op, args)
        assert not np.any(buf != 7.0)

    for o, other in (owners, owners[::-1]):
        assert o.fn("constant_host")(o.h, dp(wc)) == OK and o.fn("seek")(o.h, 5) == OK
        assert o.state(V) == (ba.WRENCH_CONSTANT, 5, wc.tobytes())
        for op, args in null_handle:
            refuse(o, other, V, op, args, None)
        for op, args in under_constant:
            refuse(o, other, V, op, args, o.h)
        assert o.fn("periodic")(o.h, 1, 6.0, 0.0, 1.0, 3.0) == OK and o.fn("mode")(o.h) == ba.WRENCH_PERIODIC
        for op, args in under_dphi_1:
            refuse(o, other, V, op, args, o.h)
        # a periodic setting that the counter's tick does not admit leaves the constant generator in force
        assert o.fn("constant_host")(o.h, dp(wc)) == OK and o.fn("seek")(o.h, EDGE) == OK
        for op, args in at_the_edge:
            refuse(o, other, V, op, args, o.h)
        assert o.state(V) == (ba.WRENCH_CONSTANT, EDGE, wc.tobytes())
        assert o.fn("periodic")(o.h, 1, 6.0, 0.0, 1.0, 3.0) == OK     # ... and the same setting in range is taken at the same tick
    f.close(); sf.close(); s.close()
    # every refusal writes a text that begins with the entry point's name
    assert not no_text, no_text


# ---- 2. steps at the edge of the periodic range -------------------------------------------------------------------------------------------
def test_steps_at_the_edge(ba):
    from bluerov2_amd.solver import _load
    L = _load()
    # the solver
    s, x0 = _solver(ba)
    e = _ekf(ba, B)
    s.set_plant_wrench(periodic=dict(dphi=1.0)); s.plant_wrench_seek(EDGE)
    assert L.brov_plant_step(s._h, 0.05, 1, None) == OK              # the step at the edge runs, the next one would leave the range
    assert L.brov_plant_step(s._h, 0.05, 1, None) == ERR_ARG and L.brov_last_error().decode().startswith("brov_plant_step")
    assert s.plant_wrench_tick() == EDGE + 1
    s.set_x0(x0); s.plant_wrench_seek(EDGE - 1)                       # ticks EDGE - 1 and EDGE are in range, the third is not
    u = np.full((TICKS, B, 4), 7.0); x = np.full((TICKS + 1, B, 12), 7.0); st = np.full((TICKS, B), 7, dtype=np.int32)
    w = np.full((TICKS, B, 6), 7.0); est = np.full((TICKS, B, 6), 7.0)
    for rc in (L.brov_closed_loop_ex(s._h, TICKS, LINE0, 16, 0.05, 1, dp(u), dp(x), ip(st), dp(w)),
               L.brov_closed_loop_dob(s._h, e._h, None, 0, TICKS, LINE0, 16, 0.05, 1, dp(u), dp(x), ip(st), dp(w), dp(est))):
        assert rc == ERR_ARG and L.brov_last_error().decode().startswith("brov_closed_loop")
        assert s.plant_wrench_tick() == EDGE - 1 and np.array_equal(s.get_x0(), x0)
        assert np.all(u == 7.0) and np.all(x == 7.0) and np.all(st == 7) and np.all(w == 7.0) and np.all(est == 7.0)
    assert L.brov_closed_loop_ex(s._h, TICKS - 1, LINE0, 16, 0.05, 1, dp(u), dp(x), ip(st), dp(w)) == OK    # two ticks fit
    assert s.plant_wrench_tick() == EDGE + 1 and not np.any(x[:TICKS] == 7.0)
    s.close(); e.close()
    # the fleet
    s, f, xv = _fleet(ba)
    e = _ekf(ba, V)
    f.set_wrench(periodic=dict(dphi=1.0)); f.wrench_seek(EDGE)
    assert L.brov_fleet_step(f._h, None, 0.05, 1, None) == OK
    assert L.brov_fleet_step(f._h, None, 0.05, 1, None) == ERR_ARG and L.brov_fleet_last_error().decode().startswith("brov_fleet_step")
    assert f.wrench_tick() == EDGE + 1
    f.set_state(xv); f.wrench_seek(EDGE - 1)
    x0 = s.get_x0()
    u = np.full((TICKS, V, 4), 7.0); x = np.full((TICKS + 1, V, 12), 7.0); st = np.full((TICKS, V), 7, dtype=np.int32)
    win = np.full((TICKS, V), 7, dtype=np.int32); w = np.full((TICKS, V, 6), 7.0); est = np.full((TICKS, V, 6), 7.0)
    for eh, est_p in ((e._h, dp(est)), (None, None)):
        rc = L.brov_closed_loop_fleet_dob(f._h, eh, TICKS, 0.0, TS, TS, 0.05, 1, dp(u), dp(x), ip(st), ip(win), dp(w), est_p)
        assert rc == ERR_ARG and L.brov_fleet_last_error().decode().startswith("brov_closed_loop_fleet_dob")
        assert f.wrench_tick() == EDGE - 1 and np.array_equal(f.state(), xv) and np.array_equal(s.get_x0(), x0)
        assert np.all(u == 7.0) and np.all(x == 7.0) and np.all(st == 7) and np.all(win == 7) and np.all(w == 7.0) and np.all(est == 7.0)
    f.close(); s.close(); e.close()


# ---- 3. any subset of logs ----------------------------------------------------------------------------------------------------------------
def _run_solver_loop(ba, kind, want):
    """one of the solver's loops on a fresh solver, with the HOST logs named in `want` and NULL for the others"""
    from bluerov2_amd.solver import _load
    L = _load()
    s, x0 = _solver(ba)
    e = _ekf(ba, B) if kind == "dob" else None
    seek = 0
    if kind != "ex_one_launch":
        s.set_plant_wrench(periodic=PERIODIC); seek = 20
    s.plant_wrench_seek(seek)
    logs = dict(u=np.full((TICKS, B, 4), 7.0), x=np.full((TICKS + 1, B, 12), 7.0), status=np.full((TICKS, B), 7, dtype=np.int32),
                wrench=np.full((TICKS, B, 6), 7.0))
    if kind == "dob":
        logs["est"] = np.full((TICKS, B, 6), 7.0)
    p = {k: ((ip if k == "status" else dp)(a) if k in want else None) for k, a in logs.items()}
    if kind == "dob":
        rc = L.brov_closed_loop_dob(s._h, e._h, None, 0, TICKS, LINE0, 16, 0.05, 1, p["u"], p["x"], p["status"], p["wrench"], p["est"])
    else:
        rc = L.brov_closed_loop_ex(s._h, TICKS, LINE0, 16, 0.05, 1, p["u"], p["x"], p["status"], p["wrench"])
    assert rc == OK, L.brov_last_error().decode()
    assert s.last_kernel_path() == ba.PATH_FUSED
    end = dict(state=s.get_x0(), tick=s.plant_wrench_tick() - seek, params=s.get_params(), results=s.results(), start=x0,
               off=s.plant_wrench_mode() == ba.WRENCH_OFF)
    if e is not None:
        end["ekf"] = np.concatenate([a.ravel() for a in e.state()])
        e.close()
    s.close()
    return logs, end


def _run_fleet_loop(ba, kind, want, ticks=TICKS):
    """one of the fleet's loops on a fresh fleet: "fleet" = brov_closed_loop_fleet under the periodic wrench, "fleet_dob" = with an
    observer under it, "fleet_dob_no_observer" = brov_closed_loop_fleet_dob without one, mode OFF"""
    from bluerov2_amd.fleet import _fleet_lib
    L = _fleet_lib()
    s, f, xv = _fleet(ba)
    e = _ekf(ba, V) if kind == "fleet_dob" else None
    seek = 0
    if kind != "fleet_dob_no_observer":
        f.set_wrench(periodic=PERIODIC); seek = 20
    f.wrench_seek(seek)
    logs = dict(u=np.full((ticks, V, 4), 7.0), x=np.full((ticks + 1, V, 12), 7.0), status=np.full((ticks, V), 7, dtype=np.int32),
                winner=np.full((ticks, V), 7, dtype=np.int32))
    if kind != "fleet":
        logs["wrench"] = np.full((ticks, V, 6), 7.0)
    if kind == "fleet_dob":
        logs["est"] = np.full((ticks, V, 6), 7.0)
    p = {k: ((ip if k in ("status", "winner") else dp)(a) if k in want else None) for k, a in logs.items()}
    if kind == "fleet":
        rc = L.brov_closed_loop_fleet(f._h, ticks, 0.0, TS, TS, 0.05, 1, p["u"], p["x"], p["status"], p["winner"])
    else:
        rc = L.brov_closed_loop_fleet_dob(f._h, e._h if e else None, ticks, 0.0, TS, TS, 0.05, 1, p["u"], p["x"], p["status"], p["winner"],
                                          p["wrench"], p.get("est"))
    assert rc == OK, L.brov_fleet_last_error().decode()
    end = dict(state=f.state(), tick=f.wrench_tick() - seek, params=s.get_params(), results=s.results(), start=xv,
               off=f.wrench_mode() == ba.WRENCH_OFF)
    if e is not None:
        end["ekf"] = np.concatenate([a.ravel() for a in e.state()])
        e.close()
    f.close(); s.close()
    return logs, end


@pytest.mark.parametrize("kind", ["ex_one_launch", "ex_per_step", "dob", "fleet", "fleet_dob", "fleet_dob_no_observer"])
def test_any_subset_of_logs(ba, kind):
    run = _run_fleet_loop if kind.startswith("fleet") else _run_solver_loop
    full, end = run(ba, kind, ("u", "x", "status", "winner", "wrench", "est"))
    assert not any(np.any(a == 7) for a in full.values()), "a log that was asked for came back with sentinels"
    assert end["tick"] == TICKS
    assert np.array_equal(full["x"][0], end["start"]) and np.array_equal(full["x"][TICKS], end["state"])
    assert not np.array_equal(full["x"][1], full["x"][0])
    if "wrench" in full:
        assert (not full["wrench"].any()) if end["off"] else np.abs(full["wrench"]).max() > 1.0
    for name in full:
        lone, lone_end = run(ba, kind, (name,))
        assert lone[name].tobytes() == full[name].tobytes(), (kind, name)
        for other in lone:
            assert other == name or np.all(lone[other] == 7), (kind, name, other, "written without being asked for")
        for k in end:
            assert np.asarray(lone_end[k]).tobytes() == np.asarray(end[k]).tobytes(), (kind, name, k)
    # no log at all: the same end
    _, none_end = run(ba, kind, ())
    for k in end:
        assert np.asarray(none_end[k]).tobytes() == np.asarray(end[k]).tobytes(), (kind, "no log", k)


@pytest.mark.parametrize("kind", ["fleet", "fleet_dob", "fleet_dob_no_observer"])
def test_fleet_loop_of_no_ticks_writes_the_start_state_alone(ba, kind):
    logs, end = _run_fleet_loop(ba, kind, ("u", "x", "status", "winner", "wrench", "est"), ticks=0)
    assert logs["x"].shape == (1, V, 12) and np.array_equal(logs["x"][0], end["start"])
    assert end["tick"] == 0 and np.array_equal(end["state"], end["start"])


# ---- 4. the solver's wrench buffers in brov_device_bytes() ----------------------------------------------------------------------------------
def test_device_bytes_grow_once_on_first_use(ba):
    tab = np.arange(24, dtype=np.float64).reshape(4, 6)
    s, _ = _solver(ba)
    d0 = s.device_bytes
    s.set_plant_wrench(constant=np.ones(6))
    assert s.device_bytes == d0 + B * 48
    s.set_plant_wrench(constant=np.zeros((B, 6)))
    assert s.device_bytes == d0 + B * 48
    s.set_plant_wrench(table=tab, gain=np.ones(B))
    assert s.device_bytes == d0 + B * 48 + B * 8
    s.set_plant_wrench(table=tab)
    s.set_plant_wrench(table=tab[:2], gain=np.ones(B))
    assert s.device_bytes == d0 + B * 48 + B * 8
    assert np.array_equal(s.plant_wrench(1), np.tile(tab[1], (B, 1)))
    assert s.device_bytes == d0 + 2 * B * 48 + B * 8
    s.plant_wrench(2); s.plant_wrench_off(); s.plant_wrench(0)
    assert s.device_bytes == d0 + 2 * B * 48 + B * 8
    s.close()
    fresh, _ = _solver(ba)
    assert fresh.device_bytes == d0
    # the first use may as well be the evaluation, or a table without a gain: each buffer still appears once
    assert not fresh.plant_wrench(3).any() and fresh.device_bytes == d0 + B * 48
    fresh.set_plant_wrench(table=tab)
    assert fresh.device_bytes == d0 + B * 48
    fresh.close()


# ---- 5. the tracked loop through the shared log -----------------------------------------------------------------------------------------------
def test_tracked_loop_in_chunks_equals_the_logged_loop(ba):
    """brov_closed_loop_track in chunks of 2 over 3 ticks under the periodic wrench: device-only columns with lead 0.  Its record is the
    one tests/track_restatement.py accumulates from the logs of the logged loop: integers and maxima exactly, sums at relative 1e-12
    (the bound derived in tests/test_gpu_track.py: n terms in another order differ by about n 2^-53, n = 3 here)."""
    a, _ = _solver(ba); b, _ = _solver(ba)
    for s in (a, b):
        s.set_plant_wrench(periodic=PERIODIC); s.plant_wrench_seek(20)
    t = ba.BatchTrack(B)
    a.closed_loop_track(t, TICKS, line0=LINE0, chunk=2)
    ul, xl, sl, wl = b.closed_loop(TICKS, line0=LINE0, log_wrench=True)
    assert a.get_x0().tobytes() == b.get_x0().tobytes() and a.results().tobytes() == b.results().tobytes()
    assert a.plant_wrench_tick() == b.plant_wrench_tick() == 20 + TICKS and np.abs(wl).max() > 1.0
    got, want = t.stats(), TrackRestatement(B).accumulate(xl[1:], ul, sl, _traj(), LINE0 + 1).stats()
    for k in ("max_pos2", "max_yaw", "ticks", "failed", "saturated", "nonfinite", "first_failed", "worst_tick", "pad_"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    for k in ("sum_pos2", "sum_yaw2", "sum_u2"):
        print(f"{k}: worst relative difference {(np.abs(got[k] - want[k]) / np.maximum(np.abs(want[k]), 1e-300)).max():.2e}")
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    assert (got["ticks"] == TICKS).all()
    a.close(); b.close(); t.close()
