"""The range stage against a triangle mesh (include/bluerov2_nmpc_mesh.h, brov_mesh_*) in numpy: the yardstick of
tests/test_mesh_restatement_cpu.py and tests/test_gpu_mesh.py, and what scripts/inspect_mesh_cpu_scenarios.py flies.  Written from the
formulas of the two headers, not from the kernel: BRUTE FORCE over all triangles, vectorised over rays x triangles; it knows nothing of the
acceleration structure, whose only contract is this result.  Every operation here is one IEEE double operation, as on the device, so depths,
hits and the mean are bit for bit given the same rotation (the device's own in the GPU tests)."""
import numpy as np

from inspect_restatement import SLOT_RANGE, noise


def stored(tri):
    """(v0, e1, e2), each [T, 3]: what the host stores of the triangles tri [T, 3, 3]; a triangle whose rounded cross product e1 x e2 is zero
    is stored with e1 = e2 = 0"""
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3)
    v0, e1, e2 = tri[:, 0].copy(), tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = _cross(e1, e2)
    dead = np.all(n == 0.0, axis=-1)
    e1[dead], e2[dead] = 0.0, 0.0
    return v0, e1, e2


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def rays(rot, p, cam):
    """(o [3], D [Q, 3], a [Q], b [Q]) of the camera at position p under the rotation rot [9]: the rays of bluerov2_nmpc_inspect.h"""
    R = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    roi, half = int(cam.roi), int(cam.roi) // 2
    q = np.arange(roi * roi)
    j = q // roi
    i = q - j * roi
    a = (((i - half) + 0.5) - cam.cx) / cam.f
    b = (((j - half) + 0.5) - cam.cy) / cam.f
    m = [cam.mount[0], cam.mount[1], cam.mount[2]]
    o = np.array([p[c] + ((R[c, 0] * m[0] + R[c, 1] * m[1]) + R[c, 2] * m[2]) for c in range(3)])
    D = np.stack([(R[c, 0] + R[c, 1] * (-a)) + R[c, 2] * (-b) for c in range(3)], axis=-1)
    return o, D, a, b


def box_depth(o, D, cam, lo, hi):
    """[Q] the smallest hit tn over the boxes, inf: none (the slab test of bluerov2_nmpc_inspect.h)"""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1, 3), np.asarray(hi, dtype=np.float64).reshape(-1, 3)
    best = np.full(len(D), np.inf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = 1.0 / D
        for k in range(len(lo)):
            tn, tf = np.full(len(D), -np.inf), np.full(len(D), np.inf)
            for c in range(3):
                t1, t2 = (lo[k, c] - o[c]) * inv[:, c], (hi[k, c] - o[c]) * inv[:, c]
                tn = np.fmax(tn, np.fmin(t1, t2))
                tf = np.fmin(tf, np.fmax(t1, t2))
            hit = (tn <= tf) & (tn >= cam.near) & (tn <= cam.far) & (tn < best)
            best = np.where(hit, tn, best)
    return best


def mesh_uvt(o, D, st):
    """(det, u, v, t), each [Q, T]: the quantities of the ray-triangle test of every ray against every stored triangle st = (v0, e1, e2)"""
    v0, e1, e2 = st
    Dq = D[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p = _cross(Dq, e2[None])
        det = _dot(e1[None], p)
        inv = 1.0 / det
        s = (o[None, :] - v0)[None]
        u = _dot(s, p) * inv
        q = _cross(s, e1[None])
        v = _dot(Dq, q) * inv
        t = _dot(e2[None], q) * inv
    return det, u, v, t


def mesh_hits(o, D, cam, st):
    """(hit [Q, T] bool, t [Q, T]): the test's verdict; every comparison is false on a NaN"""
    det, u, v, t = mesh_uvt(o, D, st)
    with np.errstate(invalid="ignore", over="ignore"):
        hit = (det != 0.0) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t >= cam.near) & (t <= cam.far)
    return hit, t


def mesh_depth(o, D, cam, st):
    """[Q] the smallest hit t over all triangles, inf: none"""
    hit, t = mesh_hits(o, D, cam, st)
    return np.where(hit, t, np.inf).min(axis=1) if hit.shape[1] else np.full(len(D), np.inf)


def mean_of(best, a, b):
    """(range without noise, hits): lane l takes the rays l, l + 64, ... in that order; then the fixed tree"""
    ret = best < np.inf
    with np.errstate(invalid="ignore"):
        rng = np.where(ret, best, 0.0) * np.sqrt((1.0 + a * a) + b * b)
    pad = (-len(best)) % 64
    rr = np.concatenate([rng, np.zeros(pad)]).reshape(-1, 64)
    hh = np.concatenate([ret, np.zeros(pad, dtype=bool)]).reshape(-1, 64)
    s, n = np.zeros(64), np.zeros(64, dtype=np.int64)
    for row in range(len(rr)):
        s = np.where(hh[row], s + rr[row], s)
        n = n + hh[row]
    stride = 32
    while stride >= 1:
        s[:stride] = s[:stride] + s[stride:2 * stride]
        n[:stride] = n[:stride] + n[stride:2 * stride]
        stride //= 2
    return (s[0] / n[0] if n[0] > 0 else 0.0), int(n[0])


def cast(rot, p, cam, st=None, lo=(), hi=()):
    """one instance: (range without noise, hits, depth [roi * roi] with 0.0 for no return) against the stored mesh st (or None) and the boxes"""
    o, D, a, b = rays(rot, p, cam)
    best = box_depth(o, D, cam, lo, hi)
    if st is not None:
        best = np.minimum(best, mesh_depth(o, D, cam, st))
    r, n = mean_of(best, a, b)
    return r, n, np.where(best < np.inf, best, 0.0)


def range_eval(rot, x, cam, tri=None, lo=(), hi=(), sigma=None, m=0):
    """the batch: dict(range [B] with the noise, hits [B], depth [B, roi * roi]) for rot [B, 9] and the states x [B, 12] at index m"""
    B = len(x)
    st = None if tri is None else stored(tri)
    out = dict(range=np.zeros(B), hits=np.zeros(B, dtype=np.int32), depth=np.zeros((B, int(cam.roi) ** 2)))
    sg = np.broadcast_to(np.asarray(0.0 if sigma is None else sigma, dtype=np.float64), (B,))
    nz = noise(int(cam.seed), np.arange(B), int(m), SLOT_RANGE)
    for b in range(B):
        r, n, d = cast(rot[b], x[b, :3], cam, st, lo, hi)
        out["range"][b] = r + sg[b] * nz[b] if n > 0 else 0.0
        out["hits"][b], out["depth"][b] = n, d
    return out
