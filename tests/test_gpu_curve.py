"""GPU tests of the plant's thrust-curve stage (brov_curve_*, curve_shift_kernel<PART>, curve_eval_kernel) against tests/curve_restatement.py, a
solver without the stage that is stepped with the restatement's applied records, and the call sequences the loops replace.  B = 130 (two
blocks and a tail lane), N = 5, Ts = 0.05, 12 ticks; tables of K = 2, 201 (the T200 fixture) and 256 knots.  The slopes are always the
stage's own (BatchSolver.thrust_curve_table)."""
import json
import os

import numpy as np
import pytest

from oracle import trajectory_oracle as T
from curve_restatement import BASIC, DEADZONE, LINEAR, PRE_NONE, PRE_POLY, PRE_TABLE, TABLE, CurveRestatement
from delay_restatement import DelayRestatement
from rotor_restatement import RotorRestatement
from thruster_restatement import ThrusterRestatement

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, TICKS = 130, 5, 12
KINDS = {LINEAR: "linear", BASIC: "basic", DEADZONE: "deadzone", TABLE: "table"}
PRES = {PRE_NONE: "none", PRE_POLY: "poly", PRE_TABLE: "table"}
BAND = 0.07                                   # half width of the dead band as a fraction of the tables' half range S
# the plant-step tests: thrust -> PWM offset by a linear map (250 thrust units -> 50 us), 4 us steps, the T200 table, kgf -> thrust units
PWM_PER_THRUST, KGF_TO_THRUST = 0.2, 60.0
POLY_LINEAR = (0.0, 0.0, 0.0, PWM_PER_THRUST, 0.0)


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


def tables(K):
    """(S, curve (x, y, amps), pre (x, y)) for K knots, both over about [-S, S]: K = 201 the T200 fixture and its inverse's range, else drawn;
    the drawn curve of 256 knots is flat zero inside +-BAND S, as the T200's is"""
    rng = np.random.default_rng(100 + K)
    if K == 201:
        import bluerov2_amd
        d = json.load(open(os.path.join(ROOT, "tests", "golden", "t200_16v.json")))
        x, y, a = bluerov2_amd.curve_from_pwm_table(d["pwm"], d["kgf"], d["amps"])
        S = 400.0
    elif K == 2:
        S = 1.0
        x, y, a = np.array([-1.0, 1.0]), np.array([-2.0, 3.0]), np.array([7.0, 9.0])
    else:
        S = 100.0
        x = np.sort(rng.uniform(-S, S, K))
        x[0], x[-1] = -S, S
        y = np.cumsum(rng.uniform(-0.2, 1.0, K)) - 40.0               # not monotone: the lookup does not need it
        y[np.abs(x) <= BAND * S] = 0.0
        a = np.abs(y) * 3.0
    px = np.sort(rng.uniform(-S, S, K))
    px[0], px[-1] = -0.9 * S, 0.9 * S
    px = np.sort(px)
    py = np.sort(rng.uniform(-S, S, K))
    return S, (x, y, a), (px, py)


def eval_inputs(K, seed):
    """[B, 6] inputs in the tables' units: uniform over +-1.5 S with specials, values exactly on knots of either table and values inside the
    dead band mixed in"""
    S, (x, _, _), (px, _) = tables(K)
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.5 * S, 1.5 * S, (B, 6))
    u = rng.random((B, 6))
    special = np.array([0.0, -0.0, np.nan, np.nan, np.inf, -np.inf, 1e300, -1e300, 5e-324, -5e-324])
    pick = u < 0.2
    v[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    pick = (u >= 0.2) & (u < 0.3)
    v[pick] = x[rng.integers(0, K, int(pick.sum()))]
    pick = (u >= 0.3) & (u < 0.4)
    v[pick] = px[rng.integers(0, K, int(pick.sum()))]
    pick = (u >= 0.4) & (u < 0.5)
    v[pick] = rng.uniform(-BAND * S, BAND * S, int(pick.sum()))
    return v


def branch_counts(x, w):
    """how many of the values w take each way through a lookup in the knots x, and how many are NaN and infinite"""
    fin = np.isfinite(w)
    return dict(below=int((w[fin] < x[0]).sum()), above=int((w[fin] > x[-1]).sum()), knot=int(np.isin(w, x).sum()),
                between=int(((w > x[0]) & (w < x[-1]) & ~np.isin(w, x)).sum()), nan=int(np.isnan(w).sum()), inf=int(np.isinf(w).sum()))


def _solver(ba, setup):
    traj, x0, pp = setup
    s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_plant_params(pp); s.set_trajectory(traj)
    return s


@pytest.fixture(scope="module")
def setup(ba):
    """(trajectory, start states, true plant parameters), left unchanged"""
    rng = np.random.default_rng(41)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]
    x0 += rng.normal(size=(B, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
    pp = np.tile(ba.P_NOMINAL, (B, 1)); pp[:, :4] = rng.uniform(-20, 20, (B, 4))
    for a in (traj, x0, pp):
        a.setflags(write=False)
    return traj, x0, pp


def _eff():
    e = np.random.default_rng(43).uniform(0.6, 1.2, (B, 6)) * KGF_TO_THRUST
    e[3] = KGF_TO_THRUST
    return e


def _t200_on(s, observer_applied=False, eff=None):
    """the T200 chain of the plant-step tests on `s`; returns its restatement with the stage's own slopes"""
    _, (x, y, a), _ = tables(201)
    s.thrust_curve_table("curve", x, y, a)
    e = _eff() if eff is None else eff
    s.set_thrust_curve(kind="table", pre="poly", pre_poly=POLY_LINEAR, quantum=4.0, eff=e, observer_applied=observer_applied)
    return CurveRestatement(B, kind=TABLE, pre=PRE_POLY, pre_poly=POLY_LINEAR, quantum=4.0, eff=e, curve=_table_of(s, "curve"))


def _table_of(s, which):
    t = s.thrust_curve_table(which)
    if which == "curve" and not t["amps"].any() and not t["amps_slope"].any():
        t["amps"] = None
    return t


def _write_records(s, rec):
    """the records `rec` [B] into the solver's own on the device (a view of them through the CUDA array interface)"""
    import torch

    class Raw:
        __cuda_array_interface__ = {"shape": (B * rec.dtype.itemsize,), "typestr": "|u1", "data": (s.results_device_ptr(), False), "version": 2}

    assert rec.shape == (B,) and rec.dtype.itemsize == 104
    torch.cuda.synchronize()
    torch.as_tensor(Raw(), device="cuda").copy_(torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()))
    torch.cuda.synchronize()


def _ekf(ba):
    par = ba.EkfParams.default(); par.compensate_coef = 1.0; par.rotor_constant = 1.0
    for j in range(12, 24):
        par.K[j] = 0.0
    return ba.BatchEkf(B, par)


def _rls(ba):
    rp = ba.RlsParams.default(); rp.compensate_coef = 1.0; rp.rotor_constant = 1.0
    return ba.BatchRls(B, rp)


def _books(s):
    st, la = s.thrust_curve_stats(), s.thrust_curve_last()
    return b"".join(v.tobytes() for v in (st["err_sq"], st["dead_ticks"], st["charge"], la["u0"], la["wanted"], la["command"], la["thrust"])), st["steps"]


def _same_books(s, r):
    st, la = s.thrust_curve_stats(), s.thrust_curve_last()
    return (st["err_sq"].tobytes() == r.err_sq.tobytes() and st["dead_ticks"].tobytes() == r.dead_ticks.tobytes()
            and st["charge"].tobytes() == r.charge.tobytes() and st["steps"] == r.steps and la["wanted"].tobytes() == r.wanted.tobytes()
            and la["command"].tobytes() == r.last_command.tobytes() and la["thrust"].tobytes() == r.last_thrust.tobytes()
            and la["u0"].tobytes() == r.last_u0.tobytes())


# ---- 1. the stage alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 201, 256])
def test_curve_eval_every_part_and_mode_is_the_restatement_bit_for_bit(ba, setup, K):
    S, (x, y, a), (px, py) = tables(K)
    s = _solver(ba, setup)
    up = s.thrust_curve_table("curve", x, y, a)
    assert np.array_equal(up["x"], x) and np.array_equal(up["y"], y) and np.array_equal(up["amps"], a) and len(up["slope"]) == K
    assert np.array_equal(up["slope"][:-1], (y[1:] - y[:-1]) / (x[1:] - x[:-1])) and up["slope"][-1] == 0.0   # the host's own quotients
    s.thrust_curve_table("pre", px, py)
    cur, pre = _table_of(s, "curve"), _table_of(s, "pre")
    eff = np.random.default_rng(5).uniform(0.5, 1.5, (B, 6)); eff[::3] = 1.0; eff[1, 0] = 0.0; eff[1, 1] = -1.0
    dz = (BAND * S) ** 2
    hit = dict(below=0, above=0, knot=0, nan=0, inf=0)
    hit_pre, dead = dict(hit), {DEADZONE: 0, TABLE: 0}
    seed = 1000 * K
    for kind in KINDS:
        for pre_mode in PRES:
            for q in (0.0, S / 100.0):
                kw = dict(quantum=q, k=2.0 / S, kl=1.5 / S, kr=2.5 / S, dl=-dz, dr=dz, pre_poly=(1e-3 / S ** 3, -1e-2 / S ** 2, 0.05 / S, 0.9, 0.01 * S))
                s.set_thrust_curve(kind=KINDS[kind], pre=PRES[pre_mode], eff=eff, **kw)
                r = CurveRestatement(B, kind=kind, pre=pre_mode, eff=eff, curve=cur, pre_table=pre, **kw)
                before = _books(s)
                seed += 1
                v = eval_inputs(K, seed)
                for part in ("command", "thrust", "both"):
                    ro, ra = r.eval(v, part)
                    go, ga = s.thrust_curve_eval(v, part)
                    assert go.tobytes() == ro.tobytes(), (KINDS[kind], PRES[pre_mode], q, part)
                    assert ga.tobytes() == ra.tobytes(), (KINDS[kind], PRES[pre_mode], q, part)
                if kind == TABLE and pre_mode == PRE_NONE and q == 0.0:
                    for k_, n in branch_counts(x, v).items():
                        hit[k_] = hit.get(k_, 0) + n
                    f, amps = s.thrust_curve_eval(v, "thrust")
                    lo_, hi_ = v < x[0], v > x[-1]                                        # beyond the ends, +-inf included: the end knots
                    assert np.isinf(v[lo_]).any() and np.isinf(v[hi_]).any()
                    assert np.all(f[lo_] == np.where(eff == 1.0, y[0], eff * y[0])[lo_]) and np.all(f[hi_] == np.where(eff == 1.0, y[-1], eff * y[-1])[hi_])
                    assert np.all(amps[v < x[0]] == a[0]) and np.all(amps[v > x[-1]] == a[-1])
                    dead[TABLE] += int(((f == 0.0) & (v != 0.0) & (eff != 0.0)).sum())
                if kind == LINEAR and pre_mode == PRE_TABLE and q == 0.0:
                    for k_, n in branch_counts(px, v).items():
                        hit_pre[k_] = hit_pre.get(k_, 0) + n
                    w, _ = s.thrust_curve_eval(v, "command")
                    assert np.all(w[np.isfinite(v) & (v < px[0])] == py[0]) and np.all(w[np.isposinf(v)] == py[-1])
                if kind == DEADZONE and pre_mode == PRE_NONE and q == 0.0:
                    f, _ = s.thrust_curve_eval(v, "thrust")
                    inside = np.isfinite(v) & (np.abs(v) < BAND * S)
                    assert not f[inside].any() and not np.signbit(f[inside & (eff > 0.0)]).any()      # +0.0 (times a negative efficiency: -0.0)
                    dead[DEADZONE] += int((inside & (v != 0.0)).sum())
                assert _books(s) == before                             # the evaluation moved no state and no statistic
    for name, h in (("curve", hit), ("pre", hit_pre)):
        print(K, name, h)
        for k_ in ("below", "above", "knot", "nan", "inf"):
            assert h[k_] >= 20, (name, k_, h)
    print(K, "dead", dead)
    assert dead[DEADZONE] >= 20 and (dead[TABLE] >= 20 or K == 2)      # (two knots have no band)
    # the default configuration evaluates to a copy, -0 and NaN included
    s.set_thrust_curve()
    v = eval_inputs(K, 7)
    for part in ("command", "thrust", "both"):
        go, ga = s.thrust_curve_eval(v, part)
        assert go.tobytes() == v.tobytes() and not ga.any()
    assert s.thrust_curve_stats()["steps"] == 0 and s.thrust_curve_last_seconds() is None
    s.close()


# ---- 2. plant steps behind the stage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["alone", "rotors", "delay_rotors_thrusters"])
def test_twelve_plant_steps_match_the_restatement_and_a_stage_off_solver(ba, setup, chain):
    """(delay 2 ->) COMMAND (-> rotors) -> THRUST (-> thruster stage) -> model under a world wrench.  After every step the stage's books and
    applied record are bit for bit the restatement's, and x0 is bit for bit that of a solver without delay, rotors and curve whose records were
    overwritten with the restatement's applied records.  Without rotors the step is one BOTH launch, with them COMMAND, rotors, THRUST."""
    s, w = _solver(ba, setup), _solver(ba, setup)
    rotors, full = chain != "alone", chain == "delay_rotors_thrusters"
    gain = np.ones((B, 6)); gain[::3, 1] = 0.5
    for o in (s, w):
        o.set_plant_wrench(constant=[10.0, -10.0, 5.0, 0.0, 0.0, 1.0])
        if full:
            o.set_thrusters(lo=-250.0, hi=250.0, gain=gain)
    tau = np.random.default_rng(44).choice([0.0, 0.05, 0.2], (B, 6))
    if full:
        s.set_delay(2)
    if rotors:
        s.set_rotors(tau, cmd_lo=-300.0, cmd_hi=300.0)
    rc = _t200_on(s)
    assert s.thrust_curve_enabled() and not w.thrust_curve_enabled()
    rd = DelayRestatement(B, 2) if full else None
    co = s.rotor_coeffs() if rotors else None
    rr = RotorRestatement(B, co["alpha"], co["beta"], -300.0, 300.0) if rotors else None
    rt = ThrusterRestatement(B, None, -250.0, 250.0, gain) if full else None
    for k in range(TICKS):
        s.set_yref_from_trajectory(k, 16); s.solve()
        res = s.results()
        tick = s.plant_wrench_tick()
        s.plant_step(0.05, 1)
        u, t = (rd.step(res["u0"], res["thrust"]) if full else (res["u0"], res["thrust"]))
        if rotors:
            u, t = rc.step_command(u, t)
            u, t = rr.step(u, t)
            assert s.rotor_last()[1].tobytes() == t.tobytes() and s.rotor_last()[0].tobytes() == u.tobytes(), k
            au, at = rc.step_thrust(u, t, 0.05)
        else:
            au, at = rc.step_both(u, t, 0.05)
        assert _same_books(s, rc), k
        assert np.array_equal(s.results()["u0"], res["u0"])           # the solver's own records stay the commanded ones
        if full:
            a, _ = rt.step(tick, at)                                  # the thruster stage's "commanded" are the delivered thrusts
            assert np.array_equal(s.thruster_last(), a), k
        rec = res.copy(); rec["u0"] = au; rec["thrust"] = at
        _write_records(w, rec)
        w.plant_step(0.05, 1)
        assert s.get_x0().tobytes() == w.get_x0().tobytes(), k
    st = s.thrust_curve_stats()
    print(chain, "err_sq", st["err_sq"].min(), st["err_sq"].max(), "charge", st["charge"].min(), st["charge"].max(), "dead ticks", st["dead_ticks"].sum())
    assert st["steps"] == TICKS and st["err_sq"].max() > 0.0 and st["charge"].max() > 0.0
    sec = s.thrust_curve_last_seconds()
    assert 0.0 < sec[0] < 1.0 and 0.0 < sec[1] < 1.0 and (rotors or sec[0] == sec[1])
    if full:
        a, b = s.thruster_stats(), w.thruster_stats()
        assert np.array_equal(a["clip_ticks"], rt.clip_ticks) and np.array_equal(a["lost_sq"], rt.lost_sq) and a["steps"] == TICKS
        assert np.array_equal(a["clip_ticks"], b["clip_ticks"]) and a["lost_sq"].tobytes() == b["lost_sq"].tobytes()
    # reset_stats keeps the last values, reset zeroes them too
    s.thrust_curve_reset(stats_only=True)
    st = s.thrust_curve_stats()
    assert st["steps"] == 0 and not st["err_sq"].any() and not st["dead_ticks"].any() and not st["charge"].any()
    assert s.thrust_curve_last()["thrust"].tobytes() == rc.last_thrust.tobytes()
    s.thrust_curve_reset()
    assert not any(v.any() for v in s.thrust_curve_last().values())
    s.close(); w.close()


# ---- 3. the default configuration is the loop without the stage ----------------------------------------------------------------------------------
def test_default_configuration_is_the_stage_off_loop_byte_for_byte(ba, setup):
    gain = np.ones((B, 6)); gain[::4, 2] = 0.0
    off, on = _solver(ba, setup), _solver(ba, setup)
    for o in (off, on):
        o.set_plant_wrench(periodic=dict(seed=5))
        o.set_thrusters(lo=-30.0, hi=30.0, gain=gain)
    on.set_thrust_curve()
    la, lb = off.closed_loop(TICKS, line0=1, log_wrench=True), on.closed_loop(TICKS, line0=1, log_wrench=True)
    for name, a, b in zip(("u", "x", "status", "wrench"), la, lb):
        assert a.tobytes() == b.tobytes(), name
    sa, sb = off.thruster_stats(), on.thruster_stats()
    assert sa["clip_ticks"].tobytes() == sb["clip_ticks"].tobytes() and sa["lost_sq"].tobytes() == sb["lost_sq"].tobytes() and sa["steps"] == sb["steps"]
    assert off.results().tobytes() == on.results().tobytes()
    last = on.thrust_curve_last()                                    # the whole record was copied
    assert last["u0"].tobytes() == on.results()["u0"].tobytes() and last["thrust"].tobytes() == on.results()["thrust"].tobytes()
    assert last["wanted"].tobytes() == last["command"].tobytes() == last["thrust"].tobytes()
    st = on.thrust_curve_stats()
    assert not st["err_sq"].any() and not st["charge"].any() and st["steps"] == TICKS
    off.close(); on.close()


# ---- 4. the loops ----------------------------------------------------------------------------------------------------------------------------------
def _chain_on(o, observer_applied=False):
    o.set_rotors(0.1, cmd_lo=-300.0, cmd_hi=300.0)
    _t200_on(o, observer_applied=observer_applied)


def test_closed_loops_equal_the_same_ticks_call_by_call(ba, setup):
    a, b = _solver(ba, setup), _solver(ba, setup)
    for o in (a, b):
        _t200_on(o)                                                    # rotor stage off: one BOTH launch per tick
    ul, xl, sl = a.closed_loop(TICKS, line0=1)
    for k in range(TICKS):
        b.set_yref_from_trajectory(1 + k, 16); b.solve(); b.plant_step(0.05, 1)
        assert b.results()["u0"].tobytes() == ul[k].tobytes() and b.get_x0().tobytes() == xl[k + 1].tobytes(), k   # the u log is the commanded input
    assert _books(a) == _books(b) and a.thrust_curve_stats()["steps"] == TICKS and a.thrust_curve_stats()["err_sq"].max() > 0.0
    a.close(); b.close()
    # the DOB and the AMPC loop: per tick window, solve, plant step, observer from the solver, hand-off
    for ampc in (False, True):
        a, b = _solver(ba, setup), _solver(ba, setup)
        ea, eb = _ekf(ba), _ekf(ba)
        ra, rb = (_rls(ba), _rls(ba)) if ampc else (None, None)
        for o in (a, b):
            _chain_on(o, observer_applied=True)
        log = a.closed_loop_dob(ea, ra, ba.APPLY_DISTURBANCE, ticks=TICKS, line0=1)
        for k in range(TICKS):
            b.set_yref_from_trajectory(1 + k, 16); b.solve(); b.plant_step(0.05, 1)
            eb.update_from_solver(b)
            if ampc:
                rb.update_from_ekf(eb, b); rb.apply_to_solver(b, ba.APPLY_DISTURBANCE)
            else:
                eb.apply_to_solver(b)
            assert b.results()["u0"].tobytes() == log["u"][k].tobytes() and b.get_x0().tobytes() == log["x"][k + 1].tobytes(), (ampc, k)
            assert eb.state()[0][:, 12:].tobytes() == log["est"][k].tobytes(), (ampc, k)
        assert _books(a) == _books(b) and a.rotor_state().tobytes() == b.rotor_state().tobytes()
        assert a.get_params().tobytes() == b.get_params().tobytes()
        for o in (a, b, ea, eb, ra, rb):
            if o is not None:
                o.close()


def test_scored_loop_in_chunks_of_twelve_and_of_five_gives_the_same_bytes(ba, setup):
    a, b = _solver(ba, setup), _solver(ba, setup)
    ta, tb = ba.BatchTrack(B), ba.BatchTrack(B)
    for o in (a, b):
        _chain_on(o)
    a.closed_loop_track(ta, TICKS, line0=1, chunk=12)
    b.closed_loop_track(tb, TICKS, line0=1, chunk=5)                 # the books live across the chunks
    assert a.get_x0().tobytes() == b.get_x0().tobytes() and a.results().tobytes() == b.results().tobytes()
    assert _books(a) == _books(b) and a.rotor_state().tobytes() == b.rotor_state().tobytes()
    assert ta.stats().tobytes() == tb.stats().tobytes() and (ta.stats()["ticks"] == TICKS).all()
    assert a.thrust_curve_stats()["steps"] == TICKS
    for o in (a, b, ta, tb):
        o.close()


# ---- 5. what the observer is fed -------------------------------------------------------------------------------------------------------------------
def test_observer_reads_the_applied_or_the_commanded_input(ba, setup):
    """brov_ekf_update_from_solver stages thrust = allocation of the u0 it reads: with the curve's flag the curve's applied records, ahead of
    the rotor stage's flag, which is set throughout; without it the rotor's; with neither the commanded ones."""
    for curve_flag, rotor_flag in ((True, True), (False, True), (False, False)):
        s = _solver(ba, setup)
        s.set_rotors(0.1, observer_applied=rotor_flag)
        _t200_on(s, observer_applied=curve_flag)
        s.set_yref_from_trajectory(0, 16); s.solve(); s.plant_step(0.05, 1)
        srcs = dict(curve=s.thrust_curve_last()["u0"], rotor=s.rotor_last()[0], commanded=s.results()["u0"])
        want = "curve" if curve_flag else ("rotor" if rotor_flag else "commanded")
        for a_ in srcs:
            for b_ in srcs:
                assert a_ == b_ or np.abs(srcs[a_] - srcs[b_]).max() > 1e-3
        x = s.get_x0()
        inv_rc = 1.0 / 0.026546960744430276

        def alloc(u):                                                  # ekf_inputs_from_solver_kernel's expression
            return np.stack([((-u[:, 0] + u[:, 1]) + u[:, 3]) * inv_rc, ((-u[:, 0] - u[:, 1]) - u[:, 3]) * inv_rc,
                             ((u[:, 0] + u[:, 1]) - u[:, 3]) * inv_rc, ((u[:, 0] - u[:, 1]) + u[:, 3]) * inv_rc, (-u[:, 2]) * inv_rc,
                             (-u[:, 2]) * inv_rc], axis=1)
        acc = x[:, 6:] / ba.EkfParams.default().dt                    # v_prev starts at zero
        e = _ekf(ba)
        e.update_from_solver(s)
        for name, u in srcs.items():
            by_hand = _ekf(ba)
            by_hand.update(alloc(u), x, acc)
            assert (e.state()[0].tobytes() == by_hand.state()[0].tobytes()) == (name == want), (curve_flag, rotor_flag, name)
            by_hand.close()
        s.close(); e.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_way_back(ba, setup):
    traj, x0, pp = setup
    s, never, fresh = _solver(ba, setup), _solver(ba, setup), _solver(ba, setup)
    _t200_on(s)
    for o in (s, never):
        o.set_yref_from_trajectory(0, 16); o.solve(); o.plant_step(0.05, 1)
    probe = eval_inputs(201, 9)

    def snapshot():
        tabs = b"".join(v.tobytes() for w in ("curve", "pre") for v in s.thrust_curve_table(w).values())
        return (_books(s), tabs, s.thrust_curve_eval(probe, "both")[0].tobytes(), s.thrust_curve_enabled(), s.get_x0().tobytes(),
                s.plant_wrench_tick())
    before = snapshot()
    assert before[0][1] == 1 and before[3]
    _, (x, y, a), _ = tables(201)
    x256 = np.arange(257.0)
    bad_x = x.copy(); bad_x[7] = bad_x[6]
    down_x = x.copy(); down_x[[10, 11]] = down_x[[11, 10]]
    nan_y = y.copy(); nan_y[200] = np.nan
    inf_a = a.copy(); inf_a[0] = np.inf
    inf_x = x.copy(); inf_x[-1] = np.inf
    eff_nan = np.ones((B, 6)); eff_nan[B - 1, 5] = np.nan
    T_ = "brov_curve_set_table_host: "
    S_ = "brov_curve_set_host: "
    cases = [(lambda: s.thrust_curve_table("curve", x[:1], y[:1]), T_ + "K must be in"),
             (lambda: s.thrust_curve_table("curve", x256, x256), T_ + "K must be in"),
             (lambda: s.thrust_curve_table("pre", x256, x256), T_ + "K must be in"),
             (lambda: s.thrust_curve_table("curve", bad_x, y, a), T_ + "the knots are not strictly increasing"),
             (lambda: s.thrust_curve_table("pre", down_x, y), T_ + "the knots are not strictly increasing"),
             (lambda: s.thrust_curve_table("curve", x, nan_y, a), T_ + "a table value is not finite"),
             (lambda: s.thrust_curve_table("curve", x, y, inf_a), T_ + "a table value is not finite"),
             (lambda: s.thrust_curve_table("curve", inf_x, y), T_ + "a table value is not finite"),
             (lambda: s.thrust_curve_table("pre", x, y, a), T_ + "the pre table has no amps column"),
             (lambda: s.thrust_curve_table(2, x, y), T_ + "unknown table"),
             (lambda: s.set_thrust_curve(eff=eff_nan), S_ + "eff must be finite"),
             (lambda: s.set_thrust_curve(eff=np.inf), S_ + "eff must be finite"),
             (lambda: s.set_thrust_curve(kind="basic", k=np.nan), S_ + "k, kl, kr, dl and dr must be finite"),
             (lambda: s.set_thrust_curve(kind="deadzone", kr=np.inf), S_ + "k, kl, kr, dl and dr must be finite"),
             (lambda: s.set_thrust_curve(pre="poly", pre_poly=[0, 0, np.nan, 1, 0]), S_ + "a polynomial coefficient is not finite"),
             (lambda: s.set_thrust_curve(kind="deadzone", dl=1.0, dr=0.5), S_ + "dl > dr"),
             (lambda: s.set_thrust_curve(quantum=-4.0), S_ + "quantum must be finite and >= 0"),
             (lambda: s.set_thrust_curve(quantum=np.nan), S_ + "quantum must be finite and >= 0"),
             (lambda: s.set_thrust_curve(quantum=np.inf), S_ + "quantum must be finite and >= 0"),
             (lambda: s.set_thrust_curve(kind=4), S_ + "unknown kind"),
             (lambda: s.set_thrust_curve(pre=-1), S_ + "unknown pre"),
             (lambda: s.set_thrust_curve(pre="table"), S_ + "BROV_CURVE_PRE_TABLE with no pre table set"),
             (lambda: fresh.set_thrust_curve(kind="table"), S_ + "BROV_CURVE_TABLE with no curve table set"),
             (lambda: s.thrust_curve_eval(probe, 0), "brov_curve_eval_host: unknown part")]
    for call, text in cases:
        with pytest.raises(RuntimeError, match=r"failed \(-1\): " + text):
            call()
        assert snapshot() == before, text
    assert not fresh.thrust_curve_enabled() and len(fresh.thrust_curve_table("curve")["x"]) == 0
    # set again: the books start afresh, the tables stay
    s.set_thrust_curve(kind="table", pre="poly", pre_poly=POLY_LINEAR, quantum=4.0, eff=_eff())
    st = s.thrust_curve_stats()
    assert st["steps"] == 0 and not st["err_sq"].any() and not st["dead_ticks"].any() and not st["charge"].any()
    assert not any(v.any() for v in s.thrust_curve_last().values())
    assert snapshot()[1:4] == before[1:4]
    # stage off again: every launch is that of a solver that never had the stage (the one-launch loop is back)
    s.thrust_curve_off()
    assert not s.thrust_curve_enabled() and s.plant_wrench_tick() == never.plant_wrench_tick() == 1
    for o in (s, never):
        o.set_x0(x0); o.init_iterate_default()
    for name, a_, b_ in zip(("u", "x", "status"), never.closed_loop(TICKS, line0=2), s.closed_loop(TICKS, line0=2)):
        assert a_.tobytes() == b_.tobytes(), name
    assert never.results().tobytes() == s.results().tobytes()
    assert s.thrust_curve_stats()["steps"] == 0                         # and the stage saw none of those steps
    for o in (s, never, fresh):
        o.close()


# ---- 7. the fleet ----------------------------------------------------------------------------------------------------------------------------------
def test_the_fleet_refuses_a_solver_with_the_stage_on(ba):
    Bf = 4
    f_s = ba.BatchSolver(Bf, ba.SolverOptions(10, 0.05))
    f_s.set_params(ba.P_NOMINAL)
    xf = np.zeros((Bf, 12)); xf[:, 2] = -20.0
    f_s.set_x0(xf); f_s.set_candidate_params("circle", np.full(Bf, 2.0), np.full(Bf, 0.5), np.zeros(Bf))
    f_s.set_thrust_curve(kind="basic", k=1e-3)
    f = ba.Fleet(f_s, 2)
    for call in (lambda: f.step(), lambda: f.closed_loop(2, dt_ref=0.05, dt_node=0.05), lambda: f.closed_loop_dob(None, 2, dt_ref=0.05, dt_node=0.05)):
        with pytest.raises(RuntimeError, match=r"failed \(-1\): brov_.*: the thrust-curve stage .*brov_curve_set_host"):
            call()
    f_s.thrust_curve_off()
    f.step()
    f.close(); f_s.close()
