#!/usr/bin/env python3
"""Writes tests/golden/bridge2_piers.npz: the underwater part of the bridge the reference's demo flies against.

start_bridge_demo spawns bluerov2_environ/urdf/bridge2.urdf, which places meshes/bridge2.STL (74 524 triangles, 3.7 MB) under the origin
xyz = (0, 0, 0), rpy = (pi/2, 0, 0).  This script reads that file from a checkout of the reference, applies the origin (a roll of exactly
pi/2 is the exact map (x, y, z) -> (x, -z, y)) and keeps the triangles with a vertex below z = -5: the piers and the floor around them,
a few hundred triangles.  Vertex data only; the whole mesh is not committed.

    python scripts/make_mesh_fixture.py /path/to/reference [out.npz]

Stored: tri float64 [T, 3, 3] world frame; sha256 of the STL file; the count of the whole mesh; the cut."""
import hashlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Z_CUT = -5.0


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    from bluerov2_amd.mesh import load_stl
    stl = os.path.join(sys.argv[1], "bluerov2_environ", "meshes", "bridge2.STL")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "bridge2_piers.npz")
    tri = load_stl(stl, xyz=(0.0, 0.0, 0.0), rpy=(0.5 * math.pi, 0.0, 0.0))
    keep = tri[(tri[:, :, 2] < Z_CUT).any(axis=1)]
    sha = hashlib.sha256(open(stl, "rb").read()).hexdigest()
    np.savez_compressed(out, tri=keep, sha256=np.array(sha), triangles_total=np.array(len(tri)), z_cut=np.array(Z_CUT))
    print(f"{stl}: {len(tri)} triangles, sha256 {sha}")
    print(f"{out}: {len(keep)} triangles with a vertex below z = {Z_CUT}, {os.path.getsize(out)} bytes")
    print("bounds", keep.reshape(-1, 3).min(axis=0), keep.reshape(-1, 3).max(axis=0))


if __name__ == "__main__":
    main()
