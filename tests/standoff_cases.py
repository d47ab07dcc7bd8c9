"""What the tests of the stand-off term share (tests/test_standoff_cpu.py, tests/test_gpu_standoff.py): the scenes, and a pool of query points
with every case a path may hold, from which the GPU tests draw their iterates -- so that the brute-force reference is computed once per scene
on the pool and gathered, never recomputed per shape."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS = 1.0                      # the radius-sized reach of the tests [m]
INF = np.inf


def piers():
    """the reference's bridge piers below z = -5: 496 world-frame triangles"""
    return np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "bridge2_piers.npz"))["tri"], dtype=np.float64)


def one_triangle():
    return np.array([[[0.5, -1.0, -20.0], [2.5, 0.25, -19.0], [1.0, 1.5, -21.5]]])


BOX1 = (np.array([[-1.0, -2.0, -22.0]]), np.array([[1.5, 0.5, -18.0]]))


def boxes8():
    rng = np.random.default_rng(8)
    lo = rng.uniform(-6, 6, (8, 3)) + np.array([0.0, 0.0, -20.0])
    return lo, lo + rng.uniform(0.2, 2.5, (8, 3))


def pool(tri, lo=(), hi=(), seed=0, n_random=400):
    """[P, 3] query points against the triangles tri [T, 3, 3] and the boxes: random points within 3 m of the geometry's bounds and within
    RADIUS of a surface, exact vertices, points on edges and faces, points 1e-9 off a face (an exact tie between two triangles arises at
    every shared vertex), points inside a box, points metres beyond every
    reach, points at 1e6 and 1e12, and rows with NaN and with +-Inf coordinates"""
    rng = np.random.default_rng(seed)
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1, 3), np.asarray(hi, dtype=np.float64).reshape(-1, 3)
    corners = np.concatenate([tri.reshape(-1, 3), lo, hi])
    blo, bhi = corners.min(axis=0), corners.max(axis=0)
    out = [rng.uniform(blo - 3.0, bhi + 3.0, (n_random, 3))]
    if len(tri):
        k = rng.integers(0, len(tri), 200)
        w = rng.dirichlet(np.ones(3), 200)
        face = np.einsum("ij,ijk->ik", w, tri[k])
        nrm = np.cross(tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0])
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
        out += [tri[k[:60]].reshape(-1, 3)[:120],                              # exact vertices
                0.5 * (tri[k[60:120], 0] + tri[k[60:120], 1]),                 # on edges (as nearly as a double is)
                face[:80],                                                     # on faces
                face[80:140] + 1e-9 * nrm[80:140],                             # 1e-9 off a face
                face + rng.uniform(-RADIUS, RADIUS, (200, 1)) * nrm,           # within the radius of a surface
                tri[k[:20], 0] + rng.normal(size=(20, 3)) * 0.3]               # about a vertex: the regions of rules 1, 3 and 5
    if len(lo):
        j = rng.integers(0, len(lo), 40)
        out += [lo[j] + rng.uniform(0, 1, (40, 3)) * (hi[j] - lo[j]),          # inside a box: 0.0
                lo[j[:10]], hi[j[:10]],                                        # its corners
                hi[j] + rng.uniform(0, 2 * RADIUS, (40, 3))]
    mid = 0.5 * (blo + bhi)
    out += [mid + rng.normal(size=(20, 3)) * 3.0 + np.array([0.0, 0.0, 500.0]),   # far beyond every finite reach of the tests
            mid + rng.choice([-1.0, 1.0], (12, 3)) * 1e6 + rng.normal(size=(12, 3)),
            mid + rng.choice([-1.0, 1.0], (6, 3)) * 1e12]
    odd = rng.uniform(blo, bhi, (12, 3))
    odd[0, 0] = np.nan; odd[1, 2] = np.nan; odd[2] = np.nan; odd[3, 1] = -np.nan
    odd[4, 0] = INF; odd[5, 1] = -INF; odd[6] = INF; odd[7, 2] = -INF; odd[8] = [INF, -INF, 0.0]
    out.append(odd[:9])
    return np.ascontiguousarray(np.concatenate(out))


def far_rows(points, reach):
    """indices of the pool's points that lie beyond `reach` of everything for sure: the block 500 m above the geometry"""
    return np.nonzero((points[:, 2] > 400.0) & (points[:, 2] < 600.0))[0]


def paths(points, V, C, n, seed, rows=None):
    """(x [V * C, n + 1, 12], idx [V * C, n + 1]): iterates whose positions are drawn from the pool; the other columns hold numbers nobody may
    read.  Every second candidate walks the pool in order (every special point is some candidate's somewhere, as far as the shape has room),
    the last candidate lies wholly beyond every finite reach.  With rows: every position is drawn from these rows of the pool, nothing else"""
    rng = np.random.default_rng(seed)
    B, K = V * C, n + 1
    if rows is not None:
        idx = np.asarray(rows)[rng.integers(0, len(rows), (B, K))]
    else:
        idx = rng.integers(0, len(points), (B, K))
        order = np.arange(B * K) % len(points)
        idx[::2] = order.reshape(B, K)[::2]
        far = far_rows(points, RADIUS)
        idx[B - 1] = far[np.arange(K) % len(far)]
    x = np.full((B, K, 12), 1e30)
    x[:, :, :3] = points[idx]
    return x, idx
