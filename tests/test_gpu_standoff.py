"""GPU tests of the stand-off term of the fleet loop (brov_standoff_*; bluerov2_amd/csrc/standoff_kernel.hip): the distance kernel and the
re-scoring against the numpy restatement byte for byte, the device loops against the same ticks composed from their parts, off meaning off,
the refusals, and scene changes between steps.  At most 260 instances; the brute-force reference is computed once per scene on a pool of
points (standoff_cases.py) the iterates are drawn from."""
import ctypes
import functools

import numpy as np
import pytest

import clearance_restatement as CR
import fleet_restatement as FR
import standoff_cases as SC
import standoff_restatement as SR

pytestmark = pytest.mark.gpu
N, TS = 20, 0.05
ERR_ARG = -1
INF = np.inf
RADIUS = SC.RADIUS


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


NONE = (np.zeros((0, 3)), np.zeros((0, 3)))
SCENES = {"piers": lambda: (SC.piers(), *NONE), "box1": lambda: (None, *SC.BOX1), "box8": lambda: (None, *SC.boxes8()),
          "both": lambda: (SC.piers(), *SC.boxes8()), "one": lambda: (SC.one_triangle(), *NONE)}


@functools.lru_cache(maxsize=None)
def reference(scene):
    """(tri, lo, hi, points [P, 3], per-point minimum of D2 over the whole scene [P]): brute force, once per scene"""
    tri, lo, hi = SCENES[scene]()
    pts = SC.pool(tri if tri is not None else np.zeros((0, 3, 3)), lo, hi, seed=len(scene))
    pm = SR.point_min(pts, None if tri is None else SR.stored(tri), lo, hi)
    pm.setflags(write=False); pts.setflags(write=False)
    return tri, lo, hi, pts, pm


def set_scene(s, tri, lo, hi, leaf=0):
    s.set_range_scene(lo, hi)
    s.set_range_mesh(tri, leaf)


# partial last waves, candidates of one vehicle inside one wave and across waves; N = 7, 20 and one case at 40
SHAPES = [(1, 3, N), (5, 3, N), (3, 64, N), (65, 2, N), (2, 130, N), (260, 1, N), (5, 3, 7), (3, 64, 40)]


@pytest.mark.parametrize("scene", sorted(SCENES))
@pytest.mark.parametrize("V,C,n", SHAPES)
def test_s2_equals_the_restatement_byte_for_byte(ba, V, C, n, scene):
    tri, lo, hi, pts, pm = reference(scene)
    B = V * C
    s = solver(ba, B, n)
    f = ba.Fleet(s, C)
    x, idx = SC.paths(pts, V, C, n, seed=1000 * V + 10 * C + n)
    s.set_iterate(x=x)
    pmx = pm[idx]
    total = {}
    for leaf in ((1, 4, 8) if tri is not None else (0,)):
        set_scene(s, tri, lo, hi, leaf)
        for first in (0, 1, n):
            vis = {}
            for reach in (RADIUS, INF):
                f.set_standoff(RADIUS, 2.0, reach, first)
                e = SR.fold(pmx, first, reach)
                d, _ = f.standoff_eval()                                  # every stage a slice of the grid
                assert d.tobytes() == e.tobytes(), (V, C, n, scene, leaf, first, reach, np.nonzero(d != e)[0][:8], d[d != e][:4], e[d != e][:4])
                d2, _, vis[reach] = f.standoff_eval(visits=True)          # one lane walks all stages: another geometry, a second call
                assert d2.tobytes() == e.tobytes(), (V, C, n, scene, leaf, first, reach, "one slice")
                assert not np.isnan(d).any() and d.max() <= reach * reach
                assert d[B - 1] == (RADIUS * RADIUS if reach == RADIUS else e[B - 1]) and pmx[B - 1].min() > 1e4    # the last candidate is out of reach
            assert np.all(vis[RADIUS] <= vis[INF])
            assert (vis[INF] > 0).any() == (tri is not None)              # boxes are no nodes
            total[(leaf, first)] = (vis[RADIUS].sum(axis=0), vis[INF].sum(axis=0))
    if scene == "piers" and (V, C, n) == (260, 1, N):
        for key, (near, far) in sorted(total.items()):
            print(f"[standoff visits] leaf {key[0]} first {key[1]}: reach {RADIUS} m {near / B} per candidate, reach inf {far / B}")
    if B * (n + 1) > 4 * len(pts):                                        # the shape has room for the whole pool
        e0 = SR.fold(pmx, 0, INF)
        assert (e0 == 0.0).any()                                          # exact vertices and box interiors
    assert f.standoff_seconds() > 0.0
    f.close(); s.close()


def synthetic_records(V, C, seed):
    """the records of tests/test_gpu_clearance.py: costs of mixed sign, every field filled, failed candidates, costs that are not finite"""
    rng = np.random.default_rng(seed)
    B = V * C
    r = np.zeros(B, dtype=FR.RESULT_DTYPE)
    r["u0"] = rng.uniform(-20, 20, (B, 4)); r["cost"] = rng.normal(size=B) * 10; r["kkt"] = rng.uniform(0, 5, B)
    r["qp_iter"] = rng.integers(0, 9, B); r["thrust"] = rng.normal(size=(B, 6))
    r["status"] = np.where(rng.uniform(size=B) < 0.2, rng.integers(1, 5, B), 0)
    odd = rng.uniform(size=B)
    r["cost"][odd < 0.08] = np.nan; r["cost"][(odd >= 0.08) & (odd < 0.16)] = np.inf; r["cost"][(odd >= 0.16) & (odd < 0.24)] = -np.inf
    r["cost"][1::7] = np.array([0xfff8000000000123], dtype=np.uint64).view(np.float64)[0]   # NaN costs with a sign and a payload to keep
    return r


@pytest.mark.parametrize("V,C", [(5, 3), (65, 2), (2, 130)])
def test_rescoring_equals_the_restatement_and_the_select_follows(ba, V, C):
    tri, lo, hi, pts, pm = reference("both")
    s = solver(ba, V * C)
    set_scene(s, tri, lo, hi)
    f = ba.Fleet(s, C)
    x, idx = SC.paths(pts, V, C, N, seed=7 * V + C, rows=np.arange(400))  # the pool's random points: distances of every size, few of them 0
    s.set_iterate(x=x)
    r = synthetic_records(V, C, seed=100 * V + C)
    e = SR.fold(pm[idx], 1, INF)
    radius = float(np.sqrt(np.median(e)))                                 # the radius cuts through the batch, whatever its density
    assert 0.0 < radius < INF
    for weight in (3.5, INF):
        f.set_standoff(radius, weight, INF, 1)
        d, out = f.standoff_eval(r)
        assert d.tobytes() == e.tobytes()
        inside = e < radius * radius
        assert inside.any() and (~inside).any()
        eo = SR.rescore(r, e, radius, weight)
        assert out.tobytes() == eo.tobytes(), np.nonzero(out["cost"].view(np.uint64) != eo["cost"].view(np.uint64))[0][:8]
        assert out.tobytes() != r.tobytes()
        w, wr = f.select(out)
        ew, ewr = FR.select(eo, V, C)
        assert np.array_equal(w, ew) and wr.tobytes() == ewr.tobytes()
        if weight == INF:
            ok = (r["status"] == 0) & np.isfinite(r["cost"])
            assert np.all(~inside[np.arange(V)[ew >= 0] * C + ew[ew >= 0]])     # no winner inside the radius
            assert not (ok & inside & np.isfinite(eo["cost"])).any()
    f.close(); s.close()


def _device_records(r):
    import torch
    return torch.from_numpy(np.frombuffer(r.tobytes(), dtype=np.uint8).copy()).cuda()


V4, C8 = 4, 8
LOOP_RADIUS, LOOP_FIRST, LOOP_REACH = 0.45, 1, 0.6
CL_RADIUS, CL_SHIFT = 0.45, 1


def _pillars(ba):
    """the structure in the way of tests/test_gpu_clearance.py's crossing fleet: a pillar as a box_mesh on the inner circles 0.45 rad ahead of
    vehicle 0 -- where the horizon of vehicle 1, which comes up at 1 m/s, ends --, and its mirror image as a box of the scene ahead of
    vehicles 2 and 3.  The outer candidates pass it by more than the radius"""
    from bluerov2_amd.mesh import box_mesh
    return box_mesh([-1.95, -0.95, -25.0], [-1.70, -0.75, -15.0]), np.array([[1.70, 0.75, -25.0]]), np.array([[1.95, 0.95, -15.0]])


def _crossing_fleet(ba, scene=True):
    """four vehicles on circles about one centre (test_gpu_clearance.py): vehicles 1 and 3 come up at 1 m/s behind vehicles 0 and 2, which crawl
    ahead of them on the same radius; the candidates are circles of radius 2.0 ... 2.7 m"""
    B = V4 * C8
    ang = np.array([0.0, -0.3, np.pi, np.pi - 0.3])
    speed = np.array([0.2, 1.0, 0.2, 1.0])
    xv = np.zeros((V4, 12))
    xv[:, 0] = -2.0 * np.cos(ang); xv[:, 1] = -2.0 * np.sin(ang); xv[:, 2] = -20.0; xv[:, 5] = ang - 0.5 * np.pi; xv[:, 6] = speed
    s = solver(ba, B)
    s.set_candidate_params("circle", np.tile(2.0 + 0.1 * np.arange(C8), V4), np.repeat(speed, C8), np.repeat(ang, C8))
    if scene:
        set_scene(s, *_pillars(ba))
    f = ba.Fleet(s, C8)
    f.set_plant_params(np.tile(ba.P_NOMINAL, (V4, 1)))
    f.set_state(xv)
    return s, f, xv


@pytest.mark.parametrize("kind,weight,clearance", [("closed_loop", 500.0, False), ("closed_loop", INF, False), ("closed_loop_dob", 1e4, False),
                                                   ("closed_loop", 500.0, True), ("closed_loop_dob", INF, True)])
def test_the_device_loop_equals_the_loop_composed_from_its_parts(ba, kind, weight, clearance):
    ticks, t0 = 8, 0.0
    periodic = dict(seed=5, scale=4.0, phase0=0.3, dphi=0.25, tz_div=3.0)
    tri, lo, hi = _pillars(ba)
    st = SR.stored(tri)

    def run(f):
        if kind == "closed_loop_dob":
            f.set_wrench(periodic=periodic)
            L = f.closed_loop_dob(None, ticks, t0=t0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1)
            return L["u"], L["x"], L["status"], L["winner"]
        return f.closed_loop(ticks, t0=t0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1)

    # the device loop with the term on ...
    s, f, xv = _crossing_fleet(ba)
    f.set_standoff(LOOP_RADIUS, weight, LOOP_REACH, LOOP_FIRST)
    if clearance:
        f.set_clearance(CL_RADIUS, 50.0, CL_SHIFT)
    ul, xl, sl, wl = run(f)
    stats_l, plan_l, cstats_l = f.standoff_stats(), f.plan(), f.clearance_stats()
    f.close(); s.close()
    # ... the same loop with it off: somewhere the fleet has to decide differently, or this test shows nothing
    s, f, _ = _crossing_fleet(ba)
    if clearance:
        f.set_clearance(CL_RADIUS, 50.0, CL_SHIFT)
    uo, xo, so, wo = run(f)
    f.close(); s.close()
    print(f"[standoff {kind} weight={weight} clearance={clearance}] winners on:\n{wl.T}\nwinners off:\n{wo.T}\nmin_s2 {stats_l['min_s2']} "
          f"below {stats_l['below']}")
    assert not np.array_equal(wl, wo)
    # ... and composed: windows -> solve -> (clearance_eval ->) standoff_eval -> both off -> step(re-scored records) -> numpy publish and stats
    s, f, _ = _crossing_fleet(ba)
    if kind == "closed_loop_dob":
        f.set_wrench(periodic=periodic)
    plan = np.repeat(xv[:, None, :3], N + 1, axis=1)
    stats, cstats = SR.fresh_stats(V4), CR.fresh_stats(V4)
    ur, xr, sr, wr = np.empty_like(ul), np.empty_like(xl), np.empty_like(sl), np.empty_like(wl)
    xr[0] = xv
    for k in range(ticks):
        s.set_yref_candidates_tick(t0 + k * TS, TS); s.solve()
        xi = s.get_iterate()[0]
        rec = None
        if clearance:
            f.set_clearance(CL_RADIUS, 50.0, CL_SHIFT)
            d, rec = f.clearance_eval()
            f.clearance_off()
        f.set_standoff(LOOP_RADIUS, weight, LOOP_REACH, LOOP_FIRST)
        s2, out = f.standoff_eval(rec)
        f.standoff_off()                                                  # the step is today's: it selects from the records it is given
        assert s2.tobytes() == SR.s2(xi, LOOP_FIRST, LOOP_REACH, st, lo, hi).tobytes()
        dev = _device_records(out)
        f.step(dev.data_ptr(), 0.05, 1)
        ur[k], sr[k], wr[k] = f.last()
        xr[k + 1] = f.state()
        stats = SR.stats(stats, s2, wr[k], V4, C8, LOOP_RADIUS)
        if clearance:
            plan = CR.publish(plan, xi, wr[k], V4, C8, CL_SHIFT)
            cstats = CR.stats(cstats, d, wr[k], V4, C8, CL_RADIUS)
            f.set_plan(plan)
    f.close(); s.close()
    assert wl.tobytes() == wr.tobytes(), (wl.T, wr.T)
    assert sl.tobytes() == sr.tobytes() and ul.tobytes() == ur.tobytes() and xl.tobytes() == xr.tobytes()
    for key in ("last_s2", "min_s2", "below"):
        assert stats_l[key].tobytes() == stats[key].tobytes(), (key, stats_l[key], stats[key])
    if clearance:
        assert plan_l.tobytes() == plan.tobytes()
        for key in ("last_d2", "min_d2", "below"):
            assert cstats_l[key].tobytes() == cstats[key].tobytes(), (key, cstats_l[key], cstats[key])
    if weight == INF:                                                     # no winner's path comes inside the radius
        assert not stats_l["below"].any() and np.all(stats_l["min_s2"] >= LOOP_RADIUS ** 2)


def test_off_means_off(ba):
    ticks = 4
    logs = []
    for toggled in (False, True):
        s, f, _ = _crossing_fleet(ba, scene=toggled)
        assert not f.standoff_enabled()
        if toggled:
            f.set_standoff(LOOP_RADIUS, INF, LOOP_REACH, LOOP_FIRST)
            assert f.standoff_enabled()
            f.standoff_off()
            assert not f.standoff_enabled()
        with pytest.raises(RuntimeError, match="brov_standoff_eval_host: the stand-off term is off"):
            f.standoff_eval()
        logs.append(f.closed_loop(ticks, t0=0.0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1))
        s.set_yref_candidates_tick(ticks * TS, TS); s.solve()
        f.step(None, 0.05, 1)
        logs[-1] = logs[-1] + f.last() + (f.state(),)
        st = f.standoff_stats()
        assert np.all(st["last_s2"] == -1.0) and np.all(st["min_s2"] == INF) and not st["below"].any()
        f.close(); s.close()
    for a, b in zip(*logs):
        assert a.tobytes() == b.tobytes()


def test_refusals(ba):
    from bluerov2_amd.fleet import _fleet_lib
    L = _fleet_lib()
    s = solver(ba, 6)
    f = ba.Fleet(s, 3)

    def refused(rc, name="brov_standoff_set", text=""):
        err = L.brov_fleet_last_error().decode()
        assert rc == ERR_ARG and err.startswith(name + ":") and text in err, err
        assert not f.standoff_enabled()

    refused(L.brov_standoff_set(f._h, 1.0, 1.0, 1.0, 1), text="neither a box nor a mesh")       # no scene
    s.set_range_scene(*SC.BOX1)
    for radius in (0.0, -1.0, np.nan, INF, 1e200, 1e-200):                 # ... and radii whose square is +Inf or 0
        refused(L.brov_standoff_set(f._h, radius, 1.0, INF, 1))
    for weight in (0.0, -2.0, np.nan, -INF):
        refused(L.brov_standoff_set(f._h, 1.0, weight, 1.0, 1))
    for reach in (0.5, 0.0, -1.0, np.nan, np.nextafter(1.0, 0.0)):         # reach < radius, and no number
        refused(L.brov_standoff_set(f._h, 1.0, 1.0, reach, 1), text="reach >= radius")
    for first in (-1, N + 1):
        refused(L.brov_standoff_set(f._h, 1.0, 1.0, 1.0, first), text="0 <= first <= N = %d" % N)
    d = np.empty(6)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    refused(L.brov_standoff_eval_host(f._h, None, dp, None, None), "brov_standoff_eval_host", "is off")
    refused(L.brov_standoff_eval_device(f._h, None, None, ctypes.c_void_p(8), None, None, None), "brov_standoff_eval_device", "is off")
    assert L.brov_standoff_last_seconds(f._h, dp) == ERR_ARG
    with pytest.raises(RuntimeError):
        f.set_standoff(-1.0)
    assert L.brov_standoff_set(f._h, 1.0, INF, 1.0, 0) == 0 and L.brov_standoff_set(f._h, 1e-3, 1e-300, INF, N) == 0
    assert f.standoff_enabled()
    f.set_standoff(0.5)                                                    # reach=None: the radius
    s2, _ = f.standoff_eval()
    assert s2.max() <= 0.25
    f.close(); s.close()


def test_scene_changes_between_steps(ba):
    """the scene is read per step: a mesh replaced between two steps is picked up by the second (brov_mesh_set_host waits for the whole
    device before it frees the old one, so a step in flight on another stream keeps what it was launched with), and a scene that has been
    emptied makes the next step fail with its text, not with a fault"""
    import torch
    from bluerov2_amd.mesh import box_mesh
    tri_a, lo, hi = _pillars(ba)
    tri_b = box_mesh([-2.6, -1.4, -25.0], [-1.7, -0.9, -15.0])             # elsewhere along the circles
    none = np.zeros((0, 3))
    s, f, xv = _crossing_fleet(ba, scene=False)
    s.set_range_mesh(tri_a)
    f.set_standoff(LOOP_RADIUS, 500.0, 3.0, LOOP_FIRST)
    stream = torch.cuda.Stream()
    stats = SR.fresh_stats(V4)
    for k, tri in enumerate((tri_a, tri_b, tri_a)):
        s.set_range_mesh(tri, leaf=1 + 3 * k)                              # right behind a step enqueued on another stream
        s.set_yref_candidates_tick(k * TS, TS); s.solve()
        xi, r = s.get_iterate()[0], s.results()
        f.step(None, 0.05, 1, stream=stream.cuda_stream)
        e = SR.s2(xi, LOOP_FIRST, 3.0, SR.stored(tri), none, none)
        other = SR.s2(xi, LOOP_FIRST, 3.0, SR.stored(tri_b if tri is tri_a else tri_a), none, none)
        ew, _ = FR.select(SR.rescore(r, e, LOOP_RADIUS, 500.0), V4, C8)
        stats = SR.stats(stats, e, ew, V4, C8, LOOP_RADIUS)
        got = f.standoff_stats()
        assert np.array_equal(f.last()[2], ew)
        for key in ("last_s2", "min_s2", "below"):
            assert got[key].tobytes() == stats[key].tobytes(), (k, key, got[key], stats[key])
        assert got["last_s2"].tobytes() != other[np.arange(V4) * C8 + np.maximum(ew, 0)].tobytes()     # ... and not against the other mesh
    # the scene emptied under a term that is on
    s.set_range_mesh(None)
    s.set_yref_candidates_tick(3 * TS, TS); s.solve()
    before = f.state()
    with pytest.raises(RuntimeError, match="brov_fleet_step: the stand-off term is on and the solver's scene holds neither"):
        f.step(None, 0.05, 1)
    with pytest.raises(RuntimeError, match="brov_closed_loop_fleet: the stand-off term is on"):
        f.closed_loop(2, t0=0.0, dt_ref=TS, dt_node=TS, dt=0.05, substeps=1)
    with pytest.raises(RuntimeError, match="brov_standoff_eval_host: the stand-off term is on"):
        f.standoff_eval()
    assert f.state().tobytes() == before.tobytes() and f.standoff_enabled()
    s.set_range_scene(lo, hi)                                              # a box alone is a scene again
    f.step(None, 0.05, 1)
    assert f.standoff_stats()["last_s2"].min() >= 0.0 or (f.last()[2] < 0).any()
    f.close(); s.close()
