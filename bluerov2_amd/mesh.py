"""Host-side mirror of include/bluerov2_nmpc_mesh.h (ctypes): the summary of the range stage's triangle mesh (brov_mesh_*), a reader of
binary STL files with a URDF origin, and two procedural meshes.  The calls themselves are methods of BatchSolver (solver.py):
set_range_mesh, range_mesh_info, range_eval(visits=True)."""
import ctypes as C
import math

import numpy as np

MESH_MAX_TRIANGLES, MESH_DEFAULT_LEAF, MESH_MAX_LEAF = 1 << 20, 4, 8   # BROV_MESH_*


class MeshInfo(C.Structure):
    """brov_mesh_summary: the mesh in force and the shape of its hierarchy (depth: edges from the root to the deepest leaf; pad: what the
    node boxes are wider than their triangles by)"""
    _fields_ = [("triangles", C.c_int64), ("nodes", C.c_int64), ("leaves", C.c_int64), ("device_bytes", C.c_int64), ("pad", C.c_double),
                ("depth", C.c_int32), ("leaf", C.c_int32)]


def origin_matrix(rpy):
    """the rotation of a URDF origin rpy = (roll, pitch, yaw): Rz(yaw) Ry(pitch) Rx(roll).  An angle that is a multiple of pi / 2 (as a
    double) contributes exact 0 and +-1, so a roll of exactly pi / 2 is the exact map (x, y, z) -> (x, -z, y)"""
    def cs(a):
        q = a / (0.5 * math.pi)
        if q == round(q) and abs(q) < 1 << 20:
            return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(round(q)) % 4]
        return math.cos(a), math.sin(a)
    (cr, sr), (cp, sp), (cy, sy) = cs(float(rpy[0])), cs(float(rpy[1])), cs(float(rpy[2]))
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    return rz @ ry @ rx


def load_stl(path, xyz=(0.0, 0.0, 0.0), rpy=(0.0, 0.0, 0.0)):
    """[T, 3, 3] float64 world-frame triangles (triangle, vertex, xyz) of the BINARY STL file `path` (80-byte header, uint32 count, 50 bytes
    per triangle: normal, three float32 vertices, attribute) under the URDF origin xyz, rpy: world = R(rpy) v + xyz.  The normals are not
    used.  An ASCII STL file is refused"""
    raw = np.fromfile(path, dtype=np.uint8)
    if len(raw) < 84:
        raise ValueError(f"{path}: too short for a binary STL file")
    count = int(raw[80:84].view("<u4")[0])
    if len(raw) != 84 + 50 * count:
        if bytes(raw[:5]).lower() == b"solid":
            raise ValueError(f"{path}: an ASCII STL file; only binary STL is read")
        raise ValueError(f"{path}: {len(raw)} bytes do not hold the {count} triangles the header announces")
    rec = raw[84:].reshape(count, 50)[:, 12:48].copy().view("<f4").reshape(count, 3, 3).astype(np.float64)
    if not np.all(np.isfinite(rec)):
        raise ValueError(f"{path}: a coordinate is not finite")
    R = origin_matrix(rpy)
    if np.all((R == 0.0) | (np.abs(R) == 1.0)):      # a signed permutation: exact, no products of rounded sines
        idx, sign = np.argmax(np.abs(R), axis=1), R[np.arange(3), np.argmax(np.abs(R), axis=1)]
        out = rec[:, :, idx] * sign
    else:
        out = rec @ R.T
    return np.ascontiguousarray(out + np.asarray(xyz, dtype=np.float64))


def box_mesh(lo, hi):
    """[12, 3, 3]: the six faces of the axis-aligned box lo, hi, two triangles each, split along the diagonal from the face's low corner"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    tri = []
    for c in range(3):
        a, b = (c + 1) % 3, (c + 2) % 3
        for side in (lo, hi):
            def v(sa, sb):
                p = np.empty(3)
                p[c], p[a], p[b] = side[c], (hi if sa else lo)[a], (hi if sb else lo)[b]
                return p
            tri.append([v(0, 0), v(1, 0), v(1, 1)])
            tri.append([v(0, 0), v(1, 1), v(0, 1)])
    return np.array(tri)


def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """[20 * 4^level, 3, 3]: an icosahedron subdivided `level` times onto the sphere (level 3: 1280 triangles, 6: 81 920)"""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    t = v[f] / np.linalg.norm(v[0])
    for _ in range(level):
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        ab, bc, ca = a + b, b + c, c + a
        ab, bc, ca = (m / np.linalg.norm(m, axis=1, keepdims=True) for m in (ab, bc, ca))
        t = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)])
    return np.ascontiguousarray(t * radius + np.asarray(centre, dtype=np.float64))


def protos(bind, L):
    """the prototypes of the family, declared through solver.py's `_bind`"""
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    bind(L, {"brov_mesh_set_host": [vp, C.c_int64, dp, C.c_int32], "brov_mesh_info": [vp, C.POINTER(MeshInfo)],
             "brov_mesh_eval_host": [vp, C.c_int64, dp, dp, ip, dp, dp, C.POINTER(C.c_int64)]})
