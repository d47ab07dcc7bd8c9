"""GPU tests of the inter-vehicle clearance term of the fleet loop (brov_clearance_*; bluerov2_amd/csrc/clearance_kernel.hip): the distance
kernel and the re-scoring against the numpy restatement byte for byte, what a step publishes, the device loops against the same ticks
composed from their parts, off meaning off, and the argument checks.  At most 260 instances."""
import ctypes

import numpy as np
import pytest

import clearance_restatement as CR
import fleet_restatement as FR

pytestmark = pytest.mark.gpu
N, TS = 20, 0.05
ERR_ARG = -1
INF = np.inf


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


def solver(ba, B, n=N):
    s = ba.BatchSolver(B, ba.SolverOptions(n, TS))
    s.set_params(ba.P_NOMINAL)
    return s


def synthetic_records(V, C, seed):
    """the records of tests/test_gpu_fleet.py: costs of mixed sign, every field filled, a sprinkling of failed candidates -- and costs that are
    not finite"""
    rng = np.random.default_rng(seed)
    B = V * C
    r = np.zeros(B, dtype=FR.RESULT_DTYPE)
    r["u0"] = rng.uniform(-20, 20, (B, 4)); r["cost"] = rng.normal(size=B) * 10; r["kkt"] = rng.uniform(0, 5, B)
    r["qp_iter"] = rng.integers(0, 9, B); r["thrust"] = rng.normal(size=(B, 6))
    r["status"] = np.where(rng.uniform(size=B) < 0.2, rng.integers(1, 5, B), 0)
    odd = rng.uniform(size=B)
    r["cost"][odd < 0.08] = np.nan; r["cost"][(odd >= 0.08) & (odd < 0.16)] = np.inf; r["cost"][(odd >= 0.16) & (odd < 0.24)] = -np.inf
    return r


def scene(V, C, n, seed):
    """random paths and plans with the cases every shape has to hold: one vehicle's plan with NaN rows, candidate 0 lying on its own vehicle's
    plan, two peers (vehicles 1 and 2) with the same plan -- an exact tie"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(V * C, n + 1, 12)) * 3.0
    plan = rng.normal(size=(V, n + 1, 3)) * 3.0
    if V >= 3:
        plan[2] = plan[1]
    if V >= 2:
        plan[V - 1, 2:5] = np.nan
        plan[V - 1, n, 1] = np.nan
    x[0, :, :3] = plan[0]
    return x, plan


# (V, C, N, shifts).  A wavefront walks ceil(V / (4 * slices)) peers per stage: four at a time with the next four asked for ahead, then a
# tail of up to three.  With the default slice count (8 wherever V >= 29) only (260, 1) reaches a second group of four (9 = 4 + 4 + 1), so
# every shape is also run cut into 1 slice -- (65, 2): 17 = 4 x 4 + 1, (130, 1): 33 = 8 x 4 + 1, vehicles of the batch in every group -- and
# into 8, against the same restatement: the bytes do not depend on the launch geometry.  The restatement of (260, 1) costs 2.5 s per shift.
SHAPES = [(1, 3, N, (0, 1, N)), (2, 1, N, (0, 1, N)), (5, 3, N, (0, 1, N)), (3, 64, N, (0, 1, N)), (65, 2, N, (0, 1, N)),
          (130, 1, N, (0, 1, N)), (2, 130, N, (0, 1, N)), (5, 3, 7, (0, 1, 7)), (3, 64, 40, (0, 1, 40)), (260, 1, N, (1,))]


@pytest.mark.parametrize("V,C,n,shifts", SHAPES)
def test_distance_kernel_equals_the_restatement_byte_for_byte(ba, V, C, n, shifts):
    s = solver(ba, V * C, n)
    f = ba.Fleet(s, C)
    x, plan = scene(V, C, n, seed=1000 * V + 10 * C + n)
    s.set_iterate(x=x)
    f.set_plan(plan)
    assert f.plan().tobytes() == plan.tobytes()
    default = f.clearance_slices()
    assert 1 <= default <= 8 and (V < 29 or default == 8)
    for shift in shifts:
        f.set_clearance(1.0, 2.0, shift)
        e = CR.d2min(x, plan, V, C, shift)
        for slices in (0, 1, 3, 8):                                     # 0: the default
            assert f.clearance_slices(slices) == (slices or default)
            d, _ = f.clearance_eval()
            assert d.tobytes() == e.tobytes(), (V, C, n, shift, slices, np.nonzero(d != e)[0][:8], d[d != e][:4], e[d != e][:4])
        d2, _ = f.clearance_eval()
        assert d2.tobytes() == d.tobytes()                              # two calls, the same bytes
        f.clearance_slices(0)
        if V == 1:
            assert np.all(d == INF)
        else:
            assert not np.isnan(d).any()
            if shift == 0:
                assert d[0] > 0.0                                       # candidate 0 IS its vehicle's plan: the vehicle itself is no peer
    assert f.clearance_seconds() > 0.0
    f.close(); s.close()


@pytest.mark.parametrize("V,C", [(5, 3), (65, 2), (2, 130)])
def test_rescoring_equals_the_restatement_and_the_select_follows(ba, V, C):
    s = solver(ba, V * C)
    f = ba.Fleet(s, C)
    x, plan = scene(V, C, N, seed=7 * V + C)
    s.set_iterate(x=x)
    f.set_plan(plan)
    r = synthetic_records(V, C, seed=100 * V + C)
    r["cost"][1::7] = np.array([0xfff8000000000123], dtype=np.uint64).view(np.float64)[0]   # NaN costs with a sign and a payload to keep
    e = CR.d2min(x, plan, V, C, 1)
    radius = float(np.sqrt(np.median(e)))                               # the radius cuts through the batch, whatever its density
    for weight in (3.5, INF):
        f.set_clearance(radius, weight, 1)
        d, out = f.clearance_eval(r)
        assert d.tobytes() == e.tobytes()
        inside = e < radius * radius
        assert inside.any() and (~inside).any()
        eo = CR.rescore(r, e, radius, weight)
        assert out.tobytes() == eo.tobytes(), np.nonzero(out["cost"].view(np.uint64) != eo["cost"].view(np.uint64))[0][:8]
        assert out.tobytes() != r.tobytes()
        w, wr = f.select(out)
        ew, ewr = FR.select(eo, V, C)
        assert np.array_equal(w, ew) and wr.tobytes() == ewr.tobytes()
        if weight == INF:
            ok = (r["status"] == 0) & np.isfinite(r["cost"])
            assert np.all(~inside[np.arange(V)[ew >= 0] * C + ew[ew >= 0]])    # no winner inside the radius
            assert not (ok & inside & np.isfinite(eo["cost"])).any()
    f.close(); s.close()


def _device_records(r):
    import torch
    return torch.from_numpy(np.frombuffer(r.tobytes(), dtype=np.uint8).copy()).cuda()


def test_a_step_publishes_the_winners_paths_and_the_statistics(ba):
    V, C, shift, radius, weight = 5, 3, 2, 1.5, 4.0
    B = V * C
    rng = np.random.default_rng(31)
    s = solver(ba, B)
    xv = np.zeros((V, 12)); xv[:, 0] = -2.0 - 0.3 * np.arange(V); xv[:, 2] = -20.0; xv[:, 5] = -0.5 * np.pi
    s.set_candidate_params("circle", np.tile(2.0 + 0.25 * np.arange(C), V), np.full(B, 0.5), np.zeros(B))
    f = ba.Fleet(s, C)
    f.set_state(xv)
    hold = np.repeat(xv[:, None, :3], N + 1, axis=1)
    assert f.plan().tobytes() == hold.tobytes()                          # before the first step every vehicle is planned where it is
    st0 = f.clearance_stats()
    assert np.all(st0["last_d2"] == -1.0) and np.all(st0["min_d2"] == INF) and not st0["below"].any()
    plan = hold + rng.normal(size=hold.shape) * 0.2
    f.set_plan(plan)
    f.set_clearance(radius, weight, shift)
    stats = CR.fresh_stats(V)
    for tick, forced in enumerate((None, 1, 3)):                         # the second and third step: a group without a winner
        s.set_yref_candidates_tick(TS * tick, TS); s.solve()
        xi = s.get_iterate()[0]
        r = s.results()
        if forced is None:
            f.step(None, 0.05, 1)
        else:
            r["status"][forced * C:(forced + 1) * C] = 4
            dev = _device_records(r)
            f.step(dev.data_ptr(), 0.05, 1)
        d = CR.d2min(xi, plan, V, C, shift)
        ew, _, es = FR.apply(CR.rescore(r, d, radius, weight), V, C, np.zeros((V, 4)))
        u, st, w = f.last()
        assert np.array_equal(w, ew) and np.array_equal(st, es)
        assert (forced is None and np.all(w >= 0)) or w[forced] == -1
        new = CR.publish(plan, xi, ew, V, C, shift)
        got = f.plan()
        assert got.tobytes() == new.tobytes()
        for v in range(V):
            if ew[v] >= 0:
                assert np.array_equal(got[v], xi[v * C + ew[v], :, :3])
            else:
                assert np.array_equal(got[v], plan[v][np.minimum(np.arange(N + 1) + shift, N)])
        stats = CR.stats(stats, d, ew, V, C, radius)
        gs = f.clearance_stats()
        for key in ("last_d2", "min_d2", "below"):
            assert gs[key].tobytes() == stats[key].tobytes(), (tick, key, gs[key], stats[key])
        plan = new
    # a reset plans every vehicle where it is again and forgets the statistics
    f.reset()
    xr = f.state()
    assert f.plan().tobytes() == np.repeat(xr[:, None, :3], N + 1, axis=1).tobytes()
    st0 = f.clearance_stats()
    assert np.all(st0["last_d2"] == -1.0) and np.all(st0["min_d2"] == INF) and not st0["below"].any()
    assert f.clearance_enabled()                                         # the parameters survive a reset
    f.close(); s.close()


V4, C8 = 4, 8
LOOP_RADIUS, LOOP_SHIFT = 0.45, 1


def _crossing_fleet(ba):
    """four vehicles on circles about one centre: vehicles 1 and 3 come up at 1 m/s behind vehicles 0 and 2, which crawl ahead of them on the
    same radius.  The cheapest candidate of a fast vehicle is the circle it is on -- through the slow vehicle"""
    B = V4 * C8
    ang = np.array([0.0, -0.3, np.pi, np.pi - 0.3])
    speed = np.array([0.2, 1.0, 0.2, 1.0])
    xv = np.zeros((V4, 12))
    xv[:, 0] = -2.0 * np.cos(ang); xv[:, 1] = -2.0 * np.sin(ang); xv[:, 2] = -20.0; xv[:, 5] = ang - 0.5 * np.pi; xv[:, 6] = speed
    s = solver(ba, B)
    s.set_candidate_params("circle", np.tile(2.0 + 0.1 * np.arange(C8), V4), np.repeat(speed, C8), np.repeat(ang, C8))
    f = ba.Fleet(s, C8)
    f.set_plant_params(np.tile(ba.P_NOMINAL, (V4, 1)))
    f.set_state(xv)
    return s, f, xv


@pytest.mark.parametrize("kind,weight", [("closed_loop", 50.0), ("closed_loop", INF), ("closed_loop_dob", 1e4)])
def test_the_device_loop_equals_the_loop_composed_from_its_parts(ba, kind, weight):
    ticks, t0 = 8, 0.0
    periodic = dict(seed=5, scale=4.0, phase0=0.3, dphi=0.25, tz_div=3.0)

    def run(f, clearance):
        if kind == "closed_loop_dob":
            f.set_wrench(periodic=periodic)
            L = f.closed_loop_dob(None, ticks, t0=t0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1)
            return L["u"], L["x"], L["status"], L["winner"]
        return f.closed_loop(ticks, t0=t0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1)

    # the device loop with the term on ...
    s, f, xv = _crossing_fleet(ba)
    f.set_clearance(LOOP_RADIUS, weight, LOOP_SHIFT)
    ul, xl, sl, wl = run(f, True)
    plan_l, stats_l = f.plan(), f.clearance_stats()
    f.close(); s.close()
    # ... the same loop with it off: somewhere the fleet has to decide differently, or this test shows nothing
    s, f, _ = _crossing_fleet(ba)
    uo, xo, so, wo = run(f, False)
    f.close(); s.close()
    print(f"[clearance {kind} weight={weight}] winners on:\n{wl.T}\nwinners off:\n{wo.T}\nmin_d2 {stats_l['min_d2']} below {stats_l['below']}")
    assert not np.array_equal(wl, wo)
    # ... and composed: windows -> solve -> clearance_eval -> step(re-scored records) -> numpy publish -> set_plan
    s, f, _ = _crossing_fleet(ba)
    if kind == "closed_loop_dob":
        f.set_wrench(periodic=periodic)
    plan = np.repeat(xv[:, None, :3], N + 1, axis=1)
    stats = CR.fresh_stats(V4)
    ur, xr, sr, wr = np.empty_like(ul), np.empty_like(xl), np.empty_like(sl), np.empty_like(wl)
    xr[0] = xv
    for k in range(ticks):
        s.set_yref_candidates_tick(t0 + k * TS, TS); s.solve()
        f.set_clearance(LOOP_RADIUS, weight, LOOP_SHIFT)
        d, out = f.clearance_eval()
        f.clearance_off()                                               # the step is today's: it selects from the records it is given
        xi = s.get_iterate()[0]
        assert d.tobytes() == CR.d2min_fast(xi, plan, V4, C8, LOOP_SHIFT).tobytes()
        dev = _device_records(out)
        f.step(dev.data_ptr(), 0.05, 1)
        ur[k], sr[k], wr[k] = f.last()
        xr[k + 1] = f.state()
        plan = CR.publish(plan, xi, wr[k], V4, C8, LOOP_SHIFT)
        stats = CR.stats(stats, d, wr[k], V4, C8, LOOP_RADIUS)
        f.set_plan(plan)
    f.close(); s.close()
    assert wl.tobytes() == wr.tobytes(), (wl.T, wr.T)
    assert sl.tobytes() == sr.tobytes() and ul.tobytes() == ur.tobytes() and xl.tobytes() == xr.tobytes()
    assert plan_l.tobytes() == plan.tobytes()
    for key in ("last_d2", "min_d2", "below"):
        assert stats_l[key].tobytes() == stats[key].tobytes(), (key, stats_l[key], stats[key])


def test_off_means_off(ba):
    ticks = 4
    logs = []
    for toggled in (False, True):
        s, f, _ = _crossing_fleet(ba)
        assert not f.clearance_enabled()
        if toggled:
            f.set_clearance(LOOP_RADIUS, INF, LOOP_SHIFT)
            assert f.clearance_enabled()
            f.clearance_off()
            assert not f.clearance_enabled()
        with pytest.raises(RuntimeError, match="brov_clearance_eval_host"):
            f.clearance_eval()
        plan0 = f.plan()
        logs.append(f.closed_loop(ticks, t0=0.0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1))
        assert f.plan().tobytes() == plan0.tobytes()                    # steps with the term off leave the plan alone
        st = f.clearance_stats()
        assert np.all(st["last_d2"] == -1.0) and not st["below"].any()
        f.close(); s.close()
    for a, b in zip(*logs):
        assert a.tobytes() == b.tobytes()


def test_arguments(ba):
    from bluerov2_amd.fleet import _fleet_lib
    L = _fleet_lib()
    s = solver(ba, 6)
    f = ba.Fleet(s, 3)

    def refused(rc, name="brov_clearance_set"):
        assert rc == ERR_ARG and L.brov_fleet_last_error().decode().startswith(name + ":")
        assert not f.clearance_enabled()

    for radius in (0.0, -1.0, np.nan, INF, 1e200, 1e-200):               # ... and radii whose square is +Inf or 0
        refused(L.brov_clearance_set(f._h, radius, 1.0, 1))
    for weight in (0.0, -2.0, np.nan, -INF):
        refused(L.brov_clearance_set(f._h, 1.0, weight, 1))
    for shift in (-1, N + 1):
        refused(L.brov_clearance_set(f._h, 1.0, 1.0, shift))
    d = np.empty(6)
    refused(L.brov_clearance_eval_host(f._h, None, d.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None), "brov_clearance_eval_host")
    refused(L.brov_clearance_eval_device(f._h, None, None, ctypes.c_void_p(8), None, None), "brov_clearance_eval_device")
    for slices in (-1, 9):
        refused(L.brov_clearance_dev_set_slices(f._h, slices), "brov_clearance_dev_set_slices")
    with pytest.raises(RuntimeError):
        f.set_clearance(-1.0)
    with pytest.raises(ValueError):
        f.set_plan(np.zeros((2, N, 3)))
    assert L.brov_clearance_set(f._h, 1.0, INF, 0) == 0 and L.brov_clearance_set(f._h, 1e-3, 1e-300, N) == 0
    assert f.clearance_enabled()
    f.close(); s.close()
