"""The arithmetic of the fleet loop's stand-off term without a GPU.

tests/standoff_walk_main.cpp, a program with its own main, is compiled with -ffp-contract=off -fsanitize=address,undefined and run directly
(no Python in the process, no preload).  On the piers fixture, a box_mesh, one triangle and 64 identical triangles it runs the host build of
the walk (bluerov2_amd/csrc/standoff_walk.hpp) for the leaf sizes 1 ... 8 and a radius-sized and an infinite reach: byte-equal to its own
brute force, and byte-equal to tests/standoff_restatement.py's numpy values on the point sets the GPU test draws from.

The restatement itself is held to exact arithmetic (fractions.Fraction): the condition the culling argument of DESIGN.md section 4.12d needs
is |d - d_exact| < pad / 4, a quarter of the hierarchy's pad, for points near the surface."""
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import standoff_cases as SC
import standoff_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def _meshes():
    from bluerov2_amd.mesh import box_mesh
    one = SC.one_triangle()
    return {"fixture": SC.piers(), "box_mesh": box_mesh([-0.4, -0.4, -25.0], [0.4, 0.4, -15.0]), "one": one, "identical": np.repeat(one, 64, axis=0)}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("standoff_walk")
    exe = str(tmp / "standoff_walk_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", f"-I{ROOT}/bluerov2_amd/csrc", os.path.join(ROOT, "tests", "standoff_walk_main.cpp"), "-o", exe],
                   check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    got = {}
    for name, tri in _meshes().items():
        pts = SC.pool(tri, seed=11)
        tf, pf, of = (str(tmp / f"{name}.{ext}") for ext in ("tri", "pts", "out"))
        np.ascontiguousarray(tri, dtype=np.float64).tofile(tf)
        pts.tofile(pf)
        out = subprocess.run([exe, tf, pf, of, repr(SC.RADIUS)], capture_output=True, text=True, timeout=600, env=env)
        print(name, out.stdout[-3000:], out.stderr[-3000:])
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        lines = {}
        for ln in out.stdout.splitlines():
            m = re.match(r"leaf (\d) reach (\S+) => ok node_tests (\S+) tri_tests (\S+)", ln)
            if m:
                lines[(int(m.group(1)), m.group(2))] = (float(m.group(3)), float(m.group(4)))
        got[name] = dict(tri=tri, pts=pts, lines=lines, values=np.fromfile(of).reshape(2, len(pts)))
    return got


@pytest.mark.parametrize("case", ("fixture", "box_mesh", "one", "identical"))
def test_the_walk_equals_its_brute_force_and_the_restatement_byte_for_byte(runs, case):
    r = runs[case]
    assert sorted(r["lines"]) == sorted((leaf, reach) for leaf in range(1, 9) for reach in (repr(SC.RADIUS), "inf")), r["lines"]
    pm = SR.point_min(r["pts"], SR.stored(r["tri"]))
    for row, reach in enumerate((SC.RADIUS, INF)):
        want = np.minimum(np.float64(reach) * np.float64(reach), pm)
        got = r["values"][row]
        assert got.tobytes() == want.tobytes(), (case, reach, np.nonzero(got != want)[0][:8], got[got != want][:4], want[got != want][:4])
    assert not np.isnan(r["values"]).any()
    assert (r["values"][0] == 0.0).any() or case != "fixture"                 # the exact vertices
    assert (r["values"][0] == SC.RADIUS ** 2).any() and (r["values"][1] > 1e11).any()


def test_a_finite_reach_is_what_makes_the_walk_cheap(runs):
    lines = runs["fixture"]["lines"]
    for leaf in range(1, 9):
        near, far = lines[(leaf, repr(SC.RADIUS))], lines[(leaf, "inf")]
        assert near[0] <= far[0] and near[1] <= far[1]
    near, far = lines[(4, repr(SC.RADIUS))], lines[(4, "inf")]
    print(f"piers, leaf 4, per point: reach {SC.RADIUS} m {near[0]:.1f} node tests {near[1]:.1f} triangle tests; reach inf {far[0]:.1f} and {far[1]:.1f}")
    assert far[1] < 496 / 4 and near[1] < far[1] / 2                          # no brute force, and the reach halves it at least


def test_the_vectorised_restatement_is_the_sequential_one():
    tri = SC.piers()[::9]
    st = SR.stored(tri)
    lo, hi = SC.boxes8()
    pts = SC.pool(tri, lo, hi, seed=5, n_random=30)
    x, _ = SC.paths(pts, 3, 2, 4, seed=1)
    for first, reach in ((0, INF), (1, SC.RADIUS), (4, 2.5)):
        a, b = SR.s2(x, first, reach, st, lo, hi), SR.s2_sequential(x, first, reach, st, lo, hi)
        assert a.tobytes() == b.tobytes(), (first, reach, a, b)
    rules = set()
    for p in pts[:400]:
        if np.isfinite(p).all():
            for j in range(0, len(tri), 7):
                rules.add(SR.tri_d2_one(p, st[0][j], st[1][j], st[2][j])[1])
    assert rules == set(range(1, 8)), rules                                   # every Voronoi region is met


def test_hand_computed_answers():
    st = SR.stored(np.array([[[0, 0, 0], [2, 0, 0], [0, 2, 0]]], dtype=np.float64))
    pts = np.array([[0.5, 0.5, 3.0], [-1, -1, 0], [3, 0, 0], [1, -2, 0], [-1, 3, 0], [-2, 1, 0], [2, 2, 0], [0.5, 0.5, 0]], dtype=np.float64)
    d = SR.tri_d2(pts, st)[:, 0]
    assert list(d) == [9.0, 2.0, 1.0, 4.0, 2.0, 4.0, 2.0, 0.0]
    rules = [SR.tri_d2_one(p, st[0][0], st[1][0], st[2][0])[1] for p in pts]
    assert rules == [7, 1, 2, 3, 4, 5, 6, 7]
    # a degenerate stored triangle is the point v0 (rule 1)
    deg = SR.stored(np.array([[[1, 1, 1], [2, 2, 2], [3, 3, 3]]], dtype=np.float64))
    assert not deg[1].any() and not deg[2].any()
    assert SR.tri_d2(np.array([[1.0, 1.0, 3.0]]), deg)[0, 0] == 4.0
    # boxes: outside, on the face, inside
    b = SR.box_d2(np.array([[3.0, 0.5, 0.5], [1.0, 0.5, 0.5], [0.5, 0.5, 0.5], [2.0, 3.0, -2.0]]), [[0, 0, 0]], [[1, 1, 1]])[:, 0]
    assert list(b) == [4.0, 0.0, 0.0, 1.0 + 4.0 + 4.0]
    # a candidate: the minimum starts at reach2, a NaN stage is skipped, the stages below `first` are not read
    x = np.zeros((2, 3, 12)); x[:, :, :3] = [[[0.5, 0.5, 0.0], [0.5, 0.5, 2.0], [np.nan, 0.5, 0.1]], [[0.5, 0.5, 9.0]] * 3]
    assert list(SR.s2(x, 0, 4.0, st)) == [0.0, 16.0] and list(SR.s2(x, 1, 4.0, st)) == [4.0, 16.0] and list(SR.s2(x, 2, INF, st)) == [INF, 81.0]
    stt = SR.stats(SR.fresh_stats(2), np.array([0.5, 2.0, 9.0, 1.0]), np.array([0, -1], dtype=np.int32), 2, 2, radius=1.0)
    assert list(stt["last_s2"]) == [0.5, -1.0] and list(stt["min_s2"]) == [0.5, INF] and list(stt["below"]) == [1, 0]


def _exact_d(p, v0, e1, e2):
    """the exact distance rules in rationals: D2 of the closest point of the triangle (v0, v0 + e1, v0 + e2) from p, all given as doubles"""
    F = Fraction
    p, v0, e1, e2 = ([F(float(z)) for z in q] for q in (p, v0, e1, e2))
    dot = lambda u, w: u[0] * w[0] + u[1] * w[1] + u[2] * w[2]                 # noqa: E731
    a = [p[j] - v0[j] for j in range(3)]
    b = [a[j] - e1[j] for j in range(3)]
    c = [a[j] - e2[j] for j in range(3)]
    d1, d2, d3, d4, d5, d6 = dot(e1, a), dot(e2, a), dot(e1, b), dot(e2, b), dot(e1, c), dot(e2, c)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    if d1 <= 0 and d2 <= 0:
        s, t = F(0), F(0)
    elif d3 >= 0 and d4 <= d3:
        s, t = F(1), F(0)
    elif vc <= 0 and d1 >= 0 and d3 <= 0:
        s, t = d1 / (d1 - d3), F(0)
    elif d6 >= 0 and d5 <= d6:
        s, t = F(0), F(1)
    elif vb <= 0 and d2 >= 0 and d6 <= 0:
        s, t = F(0), d2 / (d2 - d6)
    elif va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        s, t = 1 - w, w
    else:
        den = 1 / (va + vb + vc)
        s, t = vb * den, vc * den
    r = [a[j] - s * e1[j] - t * e2[j] for j in range(3)]
    return dot(r, r)


def _sqrt_fraction(q, digits=40):
    """sqrt of a non-negative Fraction to `digits` decimal digits, as a Fraction"""
    scale = 10 ** (2 * digits)
    return Fraction(math.isqrt(q.numerator * scale // q.denominator), 10 ** digits)


def test_the_restatement_against_exact_arithmetic():
    tri = SC.piers()
    st = SR.stored(tri)
    ext = float((tri.reshape(-1, 3).max(axis=0) - tri.reshape(-1, 3).min(axis=0)).max())
    pad = math.ldexp(ext, -30)
    assert abs(pad - 9.6e-8) < 1e-9
    rng = np.random.default_rng(2024)
    pairs = []                                                                # (point, triangle index)
    k = rng.integers(0, len(tri), 500)
    w = rng.dirichlet(np.ones(3), 500)
    face = np.einsum("ij,ijk->ik", w, tri[k])
    nrm = np.cross(tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    for i in range(100):
        pairs.append((face[i], k[i]))                                         # on faces
        pairs.append((0.5 * (tri[k[i], 0] + tri[k[i], 2]), k[i]))             # on edges
        pairs.append((tri[k[i], i % 3], k[i]))                                # on vertices
        pairs.append((face[100 + i] + 1e-9 * nrm[100 + i], k[100 + i]))       # 1e-9 off a face
        pairs.append((face[200 + i] + rng.normal(size=3) * 4.0, k[200 + i]))  # metres away
        pairs.append((face[300 + i] + rng.normal(size=3) * 0.5, rng.integers(0, len(tri))))   # near one triangle, held to another
    worst_units, worst_err, near = 0.0, 0.0, 0
    for p, j in pairs:
        d2, _ = SR.tri_d2_one(p, st[0][j], st[1][j], st[2][j])
        assert SR.tri_d2(p[None], (st[0][j:j + 1], st[1][j:j + 1], st[2][j:j + 1]))[0, 0] == d2
        exact = _sqrt_fraction(_exact_d(p, st[0][j], st[1][j], st[2][j]))
        err = abs(Fraction(math.sqrt(float(d2))) - exact)
        M = max(np.abs(p).max(), np.abs(tri[j]).max())
        worst_units = max(worst_units, float(err / (Fraction(2) ** -53 * Fraction(float(M)))))
        worst_err = max(worst_err, float(err))
        near += float(exact) < 10.0
        assert err < Fraction(pad) / 4, (p, j, float(err), pad)
    print(f"[standoff exact] {len(pairs)} pairs ({near} within 10 m): worst |d - d_exact| = {worst_err:.3e} m = {worst_units:.3e} x 2^-53 M; "
          f"pad / 4 = {pad / 4:.3e} m")
    assert near > len(pairs) // 2
