"""The numpy restatement of the ray-triangle test (tests/mesh_restatement.py) on its own, without a GPU: the reference's bridge from the demo's
launch pose, a cube mesh against the same box, a mesh and boxes together, and the corners of the specification (degenerate triangles, both
faces, near and far)."""
import math
import os

import numpy as np

import inspect_restatement as R
import mesh_restatement as M
from bluerov2_amd import inspect as I
from bluerov2_amd.mesh import box_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH = (17.978420, 3.259887, -34.5, 0.5 * math.pi)      # the bridge demo's launch pose: x, y, z, yaw


def _fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "bridge2_piers.npz"))["tri"]


def _cam(roi=40, **kw):
    cam = I.default_range_params()
    cam.roi = roi
    for k, v in kw.items():
        setattr(cam, k, v)
    return cam


def test_the_bridge_from_the_launch_pose():
    """bridge2.STL under the URDF's origin and no further pose: the centre rays along body x meet the pier at 1.99997828 m (a brute-force cast
    over the whole mesh gave this figure; the fixture keeps the part below z = -5), inside the controller's stand-off band 1.79 +- 0.5"""
    tri = _fixture()
    assert tri.shape == (496, 3, 3) and tri.dtype == np.float64
    rot = R.rot_np(0.0, 0.0, LAUNCH[3])
    r, n, d = M.cast(rot, LAUNCH[:3], _cam(), M.stored(tri))
    d = d.reshape(40, 40)
    centre = d[19:21, 19:21]
    print("centre rays", centre.ravel(), "mean range", r, "hits", n)
    assert np.all(np.abs(centre - 1.99997828) <= 0.5e-8), centre          # the tolerance of the printed digits
    assert n == 1600 and 1.29 < r < 2.29
    # the floor lies 1.455 m below the launch pose: a ray straight down (pitch -pi/2 turns body x to world -z ... +z is up, so pitch +pi/2)
    down = R.rot_np(0.0, 0.5 * math.pi, 0.0)
    assert down[6] == -1.0
    rd, nd, dd = M.cast(down, LAUNCH[:3], _cam(), M.stored(tri))
    print("floor below", dd.reshape(40, 40)[19:21, 19:21].ravel())
    assert nd > 0 and abs(dd.reshape(40, 40)[20, 20] - 1.455) < 1e-3


def test_a_cube_mesh_against_the_same_box():
    lo, hi = np.array([2.0, -0.5, -0.5]), np.array([3.0, 0.5, 0.5])
    st = M.stored(box_mesh(lo, hi))
    cam = _cam(40, f=40.0)                                          # a wide field: rays onto three faces and past the cube
    poses = [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.3, -1.1, 0.8, 0.1, 0.3, 0.4), (5.5, 1.3, 0.9, -0.2, 0.2, 2.9), (2.5, 0.1, 3.0, 0.0, 1.3, 0.3)]
    compared = 0
    for pose in poses:
        o, D, a, b = M.rays(R.rot_np(*pose[3:]), pose[:3], cam)
        box = M.box_depth(o, D, cam, [lo], [hi])
        mesh = M.mesh_depth(o, D, cam, st)
        det, u, v, t = M.mesh_uvt(o, D, st)
        with np.errstate(invalid="ignore"):
            w = 1.0 - u - v
            eps = 1e-9
            near_tri = (u > -eps) & (v > -eps) & (w > -eps) & (t > 0)
            on_edge = (near_tri & ((np.abs(u) < eps) | (np.abs(v) < eps) | (np.abs(w) < eps))).any(axis=1)
        clean = ~on_edge
        compared += int(clean.sum())
        assert np.array_equal(box[clean] < np.inf, mesh[clean] < np.inf), pose
        both = clean & (box < np.inf)
        assert np.all(np.abs(box[both] - mesh[both]) <= 1e-12 * np.maximum(1.0, box[both])), pose
        print(pose, "rays", len(box), "clean", int(clean.sum()), "hits", int((mesh < np.inf).sum()))
        assert 0 < (mesh[clean] < np.inf).sum()
    assert compared > 4000


def test_mesh_and_boxes_together_give_the_minimum_bit_for_bit():
    tri = _fixture()
    st = M.stored(tri)
    lo, hi = np.array([I.PIER_LO, (17.97842, 4.0, -36.0)]), np.array([I.PIER_HI, (18.2, 4.6, -34.4)])   # the pier of the box scene; a plate across half the view
    cam = _cam(40)
    box_wins = mesh_wins = False
    for yaw, dx in ((LAUNCH[3], 0.0), (LAUNCH[3] + 0.4, 0.7), (LAUNCH[3] - 0.9, -1.0)):
        p = (LAUNCH[0] + dx, LAUNCH[1], LAUNCH[2])
        rot = R.rot_np(0.02, -0.03, yaw)
        _, nb, db = M.cast(rot, p, cam, None, lo, hi)
        _, nm, dm = M.cast(rot, p, cam, st)
        r2, n2, d2 = M.cast(rot, p, cam, st, lo, hi)
        want = np.minimum(np.where(db > 0, db, np.inf), np.where(dm > 0, dm, np.inf))
        want = np.where(want < np.inf, want, 0.0)
        assert d2.tobytes() == want.tobytes()
        assert n2 == int((want > 0).sum())
        box_wins |= bool(np.any((db > 0) & ((dm == 0) | (db < dm))))
        mesh_wins |= bool(np.any((dm > 0) & ((db == 0) | (dm < db))))
        # the boxes alone are inspect_restatement's
        r0, n0, d0 = R.cast(rot, p, cam, lo, hi)
        rb, _, _ = M.cast(rot, p, cam, None, lo, hi)
        assert d0.tobytes() == db.tobytes() and n0 == nb and r0 == rb
    assert box_wins and mesh_wins                                   # each is the nearer one somewhere


def test_corners_of_the_specification():
    cam = _cam(4, f=200.0)
    rot = R.rot_np(0.0, 0.0, 0.0)
    face = np.array([[[2.0, -5.0, -5.0], [2.0, 5.0, -5.0], [2.0, 0.0, 8.0]]])
    # both faces count: the same triangle with the other winding
    d1 = M.cast(rot, (0.0, 0.0, 0.0), cam, M.stored(face))[2]
    d2 = M.cast(rot, (0.0, 0.0, 0.0), cam, M.stored(face[:, ::-1]))[2]
    assert np.all(d1 == 2.0) and np.all(d2 == 2.0)
    # degenerate triangles are stored with zero edges and never hit: a repeated vertex, three collinear points, a point
    dead = np.array([[[2.0, -5.0, -5.0], [2.0, -5.0, -5.0], [2.0, 0.0, 8.0]], [[2.0, -1.0, 0.0], [2.0, 0.0, 0.0], [2.0, 2.0, 0.0]],
                     [[2.0, 0.0, 0.0]] * 3])
    v0, e1, e2 = M.stored(dead)
    assert np.all(e1 == 0.0) and np.all(e2 == 0.0)
    r, n, d = M.cast(rot, (0.0, 0.0, 0.0), cam, (v0, e1, e2))
    assert n == 0 and r == 0.0 and np.all(d == 0.0)
    # near and far are inclusive bounds on t
    for near, far, hits in ((2.0, 100.0, 16), (np.nextafter(2.0, 3.0), 100.0, 0), (0.1, 2.0, 16), (0.1, np.nextafter(2.0, 1.0), 0)):
        assert M.cast(rot, (0.0, 0.0, 0.0), _cam(4, f=200.0, near=near, far=far), M.stored(face))[1] == hits, (near, far)
    # behind the camera: t < 0 is below near
    assert M.cast(R.rot_np(0.0, 0.0, math.pi), (0.0, 0.0, 0.0), cam, M.stored(face))[1] == 0
    # a ray in the triangle's plane: det == 0, a miss
    edge_on = np.array([[[1.0, 0.0, 0.0], [3.0, 0.0, 0.0], [2.0, 1.0, 0.0]]])
    o, D, _, _ = M.rays(rot, (0.0, 0.0, 0.0), _cam(2, cx=0.5, cy=0.5))       # pixel (0, 0) looks along body x exactly
    assert np.array_equal(D[3], [1.0, 0.0, 0.0]) or np.array_equal(D[0], [1.0, 0.0, 0.0])
    hit, _ = M.mesh_hits(o, D[[k for k in range(4) if np.array_equal(D[k], [1.0, 0.0, 0.0])]], cam, M.stored(edge_on))
    assert not hit.any()
