"""The range stage against a triangle mesh on the device (brov_mesh_*; mesh_eval_kernel, inspect_mesh_tick_kernel), B = 5 and once B = 69,
against tests/mesh_restatement.py: brute force over all triangles, given the device's own rotation.

Bars.  Per-ray depths, hits, the mean range with and without noise, the controller's state, records and statistics, the logs of the loop: bit
for bit.  The hierarchy's leaf size changes no byte.  From inside a closed mesh every ray returns.  Triangle tests per ray from inside the
1280-triangle icosphere: at most T / 16 = 80 -- a condition that separates a working hierarchy from brute force, not a measurement (the host
walk needs about 6 at leaf 4)."""
import math
import os

import numpy as np
import pytest

import inspect_restatement as R
import mesh_restatement as M
from bluerov2_amd import inspect as I
from bluerov2_amd.mesh import box_mesh, icosphere

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, DT = 5, 20, 0.05
ERR_ARG = -1
CUBE_LO, CUBE_HI = np.array([2.0, -1.125, -1.125]), np.array([4.25, 1.125, 1.125])
CUBE_F = 8.0      # a = (i + 0.5) / 8: from the origin the rays i = j run along the faces' shared diagonals, i, j = +-4.5 through the corners of x = 2


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


def _solver(ba, batch=B):
    s = ba.BatchSolver(batch, ba.SolverOptions(N, DT), device=0)
    yref = np.zeros((N + 1, 16)); yref[:, :3] = [2.0, 0.0, -20.0]
    x0 = np.zeros((batch, 12)); x0[:, :3] = [2.0, 0.0, -20.0]
    s.set_x0(x0); s.set_params(ba.P_NOMINAL); s.set_yref(yref)
    return s


@pytest.fixture(scope="module")
def solver(ba):
    s = _solver(ba)
    yield s
    s.close()


@pytest.fixture(scope="module")
def piers():
    return np.load(os.path.join(ROOT, "tests", "golden", "bridge2_piers.npz"))["tri"]


def _pier_start(batch=B):
    """the demo's launch pose and poses around it"""
    x = np.zeros((batch, 12))
    x[:, :3], x[:, 5] = I.START_POSE[:3], I.START_POSE[3]
    k = np.arange(batch)
    x[:, 0] += 0.03 * (k % 11); x[:, 2] += 0.1 * (k % 7) - 0.2 * (k > 0); x[:, 5] += 0.02 * (k % 13); x[:, 3] += 0.01 * (k % 3); x[:, 4] -= 0.015 * (k % 4)
    return x


def _cases(piers):
    """name -> (triangles, states [B, 12], camera keywords)"""
    one = np.array([[[2.0, -5.0, -4.0], [2.5, 6.0, -3.0], [1.5, 0.5, 7.0]],
                    # ... and, behind the camera of every pose but 2, which looks straight at them, three degenerate ones: never hit
                    [[-2.0, -5.0, -5.0], [-2.0, -5.0, -5.0], [-2.0, 0.0, 8.0]], [[-2.0, -1.0, 0.0], [-2.0, 0.0, 0.0], [-2.0, 2.0, 0.0]],
                    [[-2.0, 0.0, 0.0]] * 3])
    x1 = np.zeros((B, 12))
    x1[1, :3] = [0.0, 4.9, 0.0]; x1[2, 5] = math.pi; x1[3, :3], x1[3, 3:6] = [0.5, 0.2, -0.1], [0.3, -0.2, 0.1]; x1[4, :3] = [1.95, 0.3, 0.3]
    xc = np.zeros((B, 12))                                           # 0: the origin, zero attitude -- the diagonals and the corners
    xc[1, :3] = [0.0, 0.25, 0.0]; xc[2, :3], xc[2, 5] = [7.0, 0.0, 0.0], math.pi; xc[3, :3] = [3.0, 0.1, -0.2]      # 3: inside the cube
    xc[4, :3], xc[4, 3:6] = [0.5, -1.0, 0.7], [0.2, 0.1, 0.3]
    xi = np.zeros((B, 12))                                           # inside the unit-2 sphere about (1, 2, 3)
    xi[:, :3] = [1.0, 2.0, 3.0]
    xi[1, :3] += [0.5, -0.3, 0.2]; xi[2, 3:6] = [0.4, 1.2, -2.0]; xi[3, :3] += [-1.2, 0.0, 0.9]; xi[3, 5] = 2.5; xi[4, 4] = -0.5 * math.pi
    return {"one": (one, x1, dict(f=60.0)), "cube": (box_mesh(CUBE_LO, CUBE_HI), xc, dict(f=CUBE_F)),
            "piers": (piers, _pier_start(), {}), "icosphere": (icosphere(3, 2.0, (1.0, 2.0, 3.0)), xi, {})}


def _cam(roi, seed=11, **kw):
    cam = I.default_range_params()
    cam.roi, cam.seed = roi, seed
    for k, v in kw.items():
        setattr(cam, k, v)
    return cam


_REF = {}


def _reference(name, roi, tri, x, rot, kw):
    """the restatement of a case, computed once (with the device's rotation of its first run) and left as it is"""
    key = (name, roi)
    if key not in _REF:
        _REF[key] = (rot.copy(), M.range_eval(rot, x, _cam(roi, **kw), tri, m=7))
    assert _REF[key][0].tobytes() == rot.tobytes()
    return _REF[key][1]


@pytest.mark.parametrize("roi", [4, 40])
@pytest.mark.parametrize("name", ["one", "cube", "piers", "icosphere"])
def test_range_against_a_mesh_bit_for_bit(ba, solver, piers, name, roi):
    s = solver
    tri, x, kw = _cases(piers)[name]
    s.set_range_scene(np.zeros((0, 3)), np.zeros((0, 3)))
    s.set_range_mesh(tri)
    s.set_range(roi=roi, seed=11, **kw)
    try:
        o = s.range_eval(7, x, rot=True, depth=True, visits=True)
        r = _reference(name, roi, tri, x, o["rot"], kw)
        print(name, roi, "hits", o["hits"], "node tests per ray", o["visits"][:, 0] / roi ** 2, "triangle tests per ray", o["visits"][:, 1] / roi ** 2)
        assert np.array_equal(o["hits"], r["hits"]), (o["hits"], r["hits"])
        assert o["depth"].tobytes() == r["depth"].tobytes(), np.abs(o["depth"] - r["depth"]).max()
        assert o["range"].tobytes() == r["range"].tobytes(), (o["range"], r["range"])
        assert np.any(o["hits"] > 0)
        # twice, and through the plain call, which casts against the mesh as well
        again = s.range_eval(7, x, rot=True, depth=True, visits=True)
        assert all(o[k].tobytes() == again[k].tobytes() for k in o)
        plain = s.range_eval(7, x, rot=True, depth=True)
        assert all(o[k].tobytes() == plain[k].tobytes() for k in plain)
        if name == "one":
            assert o["hits"][0] == roi * roi and o["hits"][2] == 0 and o["hits"][4] == 0      # facing it; looking away; nearer than near
        if name == "cube":
            d = o["depth"][0].reshape(roi, roi)
            k = np.arange(15, 25) if roi == 40 else np.arange(roi)
            assert np.all(np.abs(d[k, k] - 2.0) < 1e-15) and o["hits"][3] == roi * roi      # the diagonal rays, corner to corner; from inside
            if roi == 40:
                assert d[25, 25] == 0.0 and d[14, 14] == 0.0                                # just past the corners
        if name == "icosphere":
            assert np.all(o["hits"] == roi * roi)                                    # a closed mesh from inside: nothing leaks
            assert np.all(o["visits"][:, 1] <= 80 * roi * roi), o["visits"]          # T / 16 triangle tests per ray at the most
            assert np.all(o["visits"][:, 0] >= roi * roi)
        # with noise
        sigma = 0.01 * (1 + np.arange(B))
        s.set_range(roi=roi, seed=11, sigma=sigma, **kw)
        n = s.range_eval(9, x)
        rn = M.range_eval(o["rot"], x, _cam(roi, **kw), tri, sigma=sigma, m=9) if name != "icosphere" or roi == 4 else None
        if rn is not None:
            assert n["range"].tobytes() == rn["range"].tobytes()
        assert np.array_equal(n["hits"], o["hits"]) and np.all((n["range"] != o["range"]) == (o["hits"] > 0))
    finally:
        s.set_range_mesh(None)


def test_the_leaf_size_changes_no_byte_and_the_summary_reports_the_shape(ba, solver, piers):
    s = solver
    s.set_range_scene(np.zeros((0, 3)), np.zeros((0, 3)))
    s.set_range(roi=40, seed=11)
    try:
        for name in ("piers", "icosphere"):
            tri, x, _ = _cases(piers)[name]
            outs = {}
            for leaf in (1, 4, 8, 0):
                s.set_range_mesh(tri, leaf=leaf)
                info = s.range_mesh_info()
                outs[leaf] = s.range_eval(3, x, rot=True, depth=True, visits=True)
                print(name, "leaf", leaf, "nodes", info.nodes, "leaves", info.leaves, "depth", info.depth, "bytes", info.device_bytes,
                      "tests per ray", outs[leaf]["visits"].sum(axis=0) / (B * 1600.0))
                assert (info.triangles, info.leaf) == (len(tri), leaf or 4) and info.device_bytes == 64 * info.nodes + 72 * len(tri)
                ext = (tri.reshape(-1, 3).max(axis=0) - tri.reshape(-1, 3).min(axis=0)).max()
                assert info.pad == ext * 2.0 ** -30 and info.leaves * (leaf or 4) >= len(tri) and 2 * info.leaves - 1 == info.nodes
                if name == "icosphere" and leaf == 4:
                    assert (info.nodes, info.depth) == (1023, 9)
            for leaf in (4, 8, 0):
                assert all(outs[1][k].tobytes() == outs[leaf][k].tobytes() for k in ("range", "hits", "rot", "depth")), (name, leaf)
            assert outs[4]["visits"].tobytes() == outs[0]["visits"].tobytes()
            assert outs[1]["visits"][:, 1].sum() < outs[8]["visits"][:, 1].sum()          # ... but the work: smaller leaves test fewer triangles
    finally:
        s.set_range_mesh(None)
    info = s.range_mesh_info()
    assert (info.triangles, info.nodes, info.leaves, info.device_bytes, info.pad, info.depth, info.leaf) == (0, 0, 0, 0, 0.0, 0, 0)


def test_mesh_and_boxes_give_the_minimum_and_removing_the_mesh_restores_the_box_kernel(ba, solver, piers):
    s = solver
    x = _pier_start()
    lo, hi = np.array([I.PIER_LO, (17.97842, 4.0, -36.0)]), np.array([I.PIER_HI, (18.2, 4.6, -34.4)])
    s.set_range(roi=40, seed=11, sigma=0.02)
    s.set_range_scene(lo, hi)
    boxes = s.range_eval(4, x, rot=True, depth=True)
    with pytest.raises(Exception, match="no mesh is set"):
        s.range_eval(4, x, visits=True)
    try:
        s.set_range_mesh(piers)
        both = s.range_eval(4, x, rot=True, depth=True)
        s.set_range_scene(np.zeros((0, 3)), np.zeros((0, 3)))
        mesh = s.range_eval(4, x, rot=True, depth=True)
        s.set_range_scene(lo, hi)
    finally:
        s.set_range_mesh(None)
    inf = lambda d: np.where(d > 0, d, np.inf)   # noqa: E731
    want = np.minimum(inf(boxes["depth"]), inf(mesh["depth"]))
    assert both["depth"].tobytes() == np.where(want < np.inf, want, 0.0).tobytes()
    assert np.any(inf(boxes["depth"]) < inf(mesh["depth"])) and np.any(inf(mesh["depth"]) < inf(boxes["depth"]))
    cam = _cam(40)
    r = M.range_eval(both["rot"], x, cam, piers, lo, hi, sigma=0.02, m=4)
    assert both["range"].tobytes() == r["range"].tobytes() and np.array_equal(both["hits"], r["hits"])
    # the mesh gone: the box kernel's bytes
    after = s.range_eval(4, x, rot=True, depth=True)
    assert all(boxes[k].tobytes() == after[k].tobytes() for k in boxes)
    rb = R.range_eval(after["rot"], x, cam, lo, hi, sigma=0.02, m=4)
    assert after["range"].tobytes() == rb["range"].tobytes() and after["depth"].tobytes() == rb["depth"].tobytes()


def test_range_does_not_depend_on_the_batch(ba, solver, piers):
    x69 = _pier_start(69)
    s69 = _solver(ba, 69)
    try:
        for s in (solver, s69):
            s.set_range_scene(np.zeros((0, 3)), np.zeros((0, 3)))
            s.set_range_mesh(piers)
            s.set_range(roi=10, seed=3, sigma=0.02)
        a = solver.range_eval(5, x69[:B], rot=True, depth=True, visits=True)
        b = s69.range_eval(5, x69, rot=True, depth=True, visits=True)
        assert all(a[k].tobytes() == b[k][:B].tobytes() for k in a)
        cam = _cam(10, seed=3)
        r = M.range_eval(b["rot"], x69, cam, piers, sigma=0.02, m=5)
        assert b["depth"].tobytes() == r["depth"].tobytes() and b["range"].tobytes() == r["range"].tobytes() and np.array_equal(b["hits"], r["hits"])
    finally:
        solver.set_range_mesh(None)
        s69.close()


def _fresh(ba, piers, thrusters):
    s = _solver(ba)
    s.set_x0(_pier_start())
    s.set_range_mesh(piers)                       # a mesh and no box: a step runs
    s.set_range(sigma=0.01, seed=5)
    if thrusters:
        s.set_thrusters(lo=np.full(6, -30.0), hi=np.full(6, 30.0))
    return s


@pytest.mark.parametrize("thrusters", [False, True])
def test_step_behind_the_plant_equals_the_composed_restatement(ba, piers, thrusters):
    """teacher-forced: every tick the restatement is fed the device's state"""
    s = _fresh(ba, piers, thrusters)
    try:
        s.set_inspect()
        par, cam = I.default_inspect_params(), I.default_range_params()
        cam.seed = 5
        st, t = I.initial_state(par, B), I.initial_stats(B)
        for k in range(30):
            x_true = s.get_x0()
            m = int(s._L.brov_plant_wrench_tick(s._h))
            s.inspect_step()
            dev_state, dev_range = s.inspect_state()
            rot = s.range_eval(m, x_true, rot=True)["rot"]
            r = M.range_eval(rot, x_true, cam, piers, sigma=0.01, m=m)
            assert dev_range.tobytes() == r["range"].tobytes(), (k, dev_range, r["range"])
            st, rec, t, _ = R.control_batch(par, st, t, r["range"], x_true[:, 2], x_true[:, 5])
            assert R.same_bytes(dev_state, st), (k, dev_state, st)
            assert R.same_bytes(s.results(), rec), (k, s.results(), rec)
            s.plant_step(DT, 2)
        assert R.same_bytes(s.inspect_stats(), t)
        assert np.all(st["started"] == 1)
    finally:
        s.close()


@pytest.mark.parametrize("thrusters", [False, True])
def test_loop_equals_the_composed_calls_and_the_restatement(ba, piers, thrusters):
    a, b = _fresh(ba, piers, thrusters), _fresh(ba, piers, thrusters)
    try:
        ticks = 30
        for s in (a, b):
            s.set_inspect()
        ul, xl, sl, rl = a.closed_loop_inspect(ticks, DT, 2)
        x, u, st, r = [b.get_x0()], [], [], []
        for k in range(ticks):
            b.inspect_step()
            state, rng = b.inspect_state()
            u.append(b.results()["u0"].copy()); st.append(state["status"].copy()); r.append(rng)
            b.plant_step(DT, 2)
            x.append(b.get_x0())
        assert xl.tobytes() == np.array(x).tobytes() and ul.tobytes() == np.array(u).tobytes()
        assert sl.tobytes() == np.array(st, dtype=np.int32).tobytes() and rl.tobytes() == np.array(r).tobytes()
        assert R.same_bytes(a.inspect_stats(), b.inspect_stats()) and R.same_bytes(a.inspect_state()[0], b.inspect_state()[0])
        # the composed restatement over the logged run: the ranges from the logged states, the controller on them
        par, cam = I.default_inspect_params(), I.default_range_params()
        cam.seed = 5
        s0, t = I.initial_state(par, B), I.initial_stats(B)
        for k in range(ticks):
            rot = b.range_eval(k, xl[k], rot=True)["rot"]
            rk = M.range_eval(rot, xl[k], cam, piers, sigma=0.01, m=k)
            assert rl[k].tobytes() == rk["range"].tobytes(), k
            s0, rec, t, _ = R.control_batch(par, s0, t, rl[k], xl[k][:, 2], xl[k][:, 5])
            assert ul[k].tobytes() == rec["u0"].tobytes(), k
        assert R.same_bytes(a.inspect_stats(), t) and R.same_bytes(a.inspect_state()[0], s0)
        assert np.all(rl > 0)
    finally:
        a.close(); b.close()


def test_a_solver_that_had_a_mesh_steps_as_one_that_never_did(ba, piers):
    a, b = _solver(ba), _solver(ba)
    L = a._L
    try:
        for s in (a, b):
            s.set_x0(_pier_start())
            s.set_range(sigma=0.01, seed=5)
            s.set_inspect()
        assert L.brov_inspect_step(a._h, None) == ERR_ARG and L.brov_last_error().decode().startswith("brov_inspect_step: the scene has no box")
        b.set_range_mesh(piers)
        b.inspect_step(); b.inspect_reset(); b.inspect_reset_stats()
        b.set_range_mesh(np.zeros((0, 3, 3)))
        assert L.brov_inspect_step(b._h, None) == ERR_ARG and L.brov_last_error().decode().startswith("brov_inspect_step: the scene has no box")
        for s in (a, b):
            s.set_range_scene(np.array([I.PIER_LO]), np.array([I.PIER_HI]))
        la, lb = a.closed_loop_inspect(5, DT, 2), b.closed_loop_inspect(5, DT, 2)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(la, lb))
        assert R.same_bytes(a.inspect_stats(), b.inspect_stats()) and R.same_bytes(a.inspect_state()[0], b.inspect_state()[0])
    finally:
        a.close(); b.close()
