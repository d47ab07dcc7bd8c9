"""The range stage's triangle mesh (brov_mesh_*) without a GPU: the C ABI's symbols and declarations (include/bluerov2_nmpc_mesh.h), the
summary structure against its ctypes mirror, the refusals that need no device, the STL reader and the Python methods."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
MESH = ["brov_mesh_set_host", "brov_mesh_info", "brov_mesh_eval_host"]


def _lib():
    import bluerov2_amd
    from bluerov2_amd.solver import _load
    bluerov2_amd.build_library()
    return _load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc_mesh.h")).read(), flags=re.S)


def test_header_declares_and_library_exports_the_new_names():
    import bluerov2_amd
    bluerov2_amd.build_library()
    declared = set(re.findall(r"\b(brov_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(MESH), sorted(declared ^ set(MESH))
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split())
    assert set(n for n in exported if n.startswith("brov_mesh_")) == set(MESH)
    main = open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read()
    assert main.count('#include "bluerov2_nmpc_mesh.h"') == 1
    assert main.index('#include "bluerov2_nmpc_mesh.h"') > main.index('#include "bluerov2_nmpc_curve.h"')
    assert "brov_mesh_set_host" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    h = _header()
    assert "BROV_MESH_MAX_TRIANGLES 1048576" in h and "BROV_MESH_DEFAULT_LEAF 4" in h and "BROV_MESH_MAX_LEAF 8" in h
    # the specification of the test is in the header's comment
    full = open(os.path.join(ROOT, "include", "bluerov2_nmpc_mesh.h")).read()
    for piece in ("p = D x e2", "det = e1 . p", "u = (s . p) inv", "t = (e2 . q) inv", "det != 0", "THE RESULT IS THAT OF TESTING EVERY TRIANGLE"):
        assert piece in full, piece


def test_the_summary_matches_its_mirror():
    import bluerov2_amd
    body = re.search(r"typedef struct brov_mesh_summary \{(.*?)\} brov_mesh_summary;", _header(), flags=re.S).group(1)
    fields = [tuple(d.split()) for d in body.split(";") if d.strip()]
    names = {C.c_double: "double", C.c_int32: "int32_t", C.c_int64: "int64_t"}
    assert fields == [(names[t], n) for n, t in bluerov2_amd.MeshInfo._fields_]
    assert C.sizeof(bluerov2_amd.MeshInfo) == 48
    from bluerov2_amd import mesh as M
    assert (M.MESH_MAX_TRIANGLES, M.MESH_DEFAULT_LEAF, M.MESH_MAX_LEAF) == (1 << 20, 4, 8) and bluerov2_amd.MESH_MAX_TRIANGLES == 1 << 20


def test_null_handles_are_argument_errors_with_the_calls_own_name():
    L = _lib()
    info = __import__("bluerov2_amd").MeshInfo()
    for name, args in [("brov_mesh_set_host", (None, 0, None, 0)), ("brov_mesh_info", (None, C.byref(info))),
                       ("brov_mesh_eval_host", (None, 0) + (None,) * 6)]:
        assert getattr(L, name)(*args) == ERR_ARG, name
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())


def test_refusals_come_with_their_text_and_before_any_device_is_touched():
    """Each refusal of brov_mesh_set_host, of the eval call without a mesh and of a step with neither box nor mesh.  A solver handle needs a
    device, the checks need none: the host side (mesh_source.hpp in inspect_source.hpp, header only) is compiled into a stand-alone host
    program whose call context counts the waits and whose launchers abort (tests/mesh_refusals_main.cpp)."""
    src = os.path.join(ROOT, "tests", "mesh_refusals_main.cpp")
    exe = os.path.join(ROOT, "bluerov2_amd", "lib", "mesh_refusals")
    import bluerov2_amd
    bluerov2_amd.build_library()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", f"-I{ROOT}/include", f"-I{ROOT}/bluerov2_amd/csrc", src, "-o", exe,
                    "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(ln.split(" => ", 1) for ln in out.stdout.splitlines() if " => " in ln)
    want = {"n = -1": "0 ... BROV_MESH_MAX_TRIANGLES", "n = 2^20 + 1": "0 ... BROV_MESH_MAX_TRIANGLES", "null triangles": "null argument",
            "leaf -1": "0 ... BROV_MESH_MAX_LEAF", "leaf 9": "0 ... BROV_MESH_MAX_LEAF", "NaN": "not finite", "-inf": "not finite",
            "inf in the last": "not finite", "eval without a mesh": "no mesh is set", "eval null": "null argument",
            "neither box nor mesh": "the scene has no box", "mesh and comp > 0": "comp > 0", "null info": "null argument"}
    for case, text in want.items():
        assert case in lines and lines[case].startswith("-1 brov_mesh_test: ") and text in lines[case], (case, lines.get(case))
    assert lines["waits"] == "0" and lines["allocations"] == "0"


def _write_stl(path, tri):
    with open(path, "wb") as f:
        f.write(b"binary stl written by a test".ljust(80, b" "))
        f.write(struct.pack("<I", len(tri)))
        for t in tri:
            f.write(struct.pack("<12fH", 0.0, 0.0, 0.0, *np.asarray(t, dtype=np.float32).ravel(), 0))


def test_load_stl_reads_binary_applies_the_origin_and_refuses_ascii(tmp_path):
    from bluerov2_amd.mesh import box_mesh, load_stl
    tri = box_mesh([0.5, -1.25, 2.0], [1.5, 0.75, 5.125])          # 12 triangles, coordinates exact in float32
    assert tri.shape == (12, 3, 3)
    p = str(tmp_path / "box.stl")
    _write_stl(p, tri)
    got = load_stl(p)
    assert got.dtype == np.float64 and got.shape == (12, 3, 3) and np.array_equal(got, tri)
    # a roll of exactly pi / 2 is the exact map (x, y, z) -> (x, -z, y), whatever the coordinates
    odd = tri * np.float32(1.1)
    _write_stl(p, odd)
    base = load_stl(p)
    rolled = load_stl(p, rpy=(0.5 * math.pi, 0.0, 0.0))
    assert np.array_equal(rolled, np.stack([base[..., 0], -base[..., 2], base[..., 1]], axis=-1))
    moved = load_stl(p, xyz=(1.0, -2.0, 0.5), rpy=(0.5 * math.pi, 0.0, 0.0))
    assert np.array_equal(moved, rolled + np.array([1.0, -2.0, 0.5]))
    # a general origin: the URDF's fixed-axis roll-pitch-yaw
    r, pt, y = 0.3, -0.2, 1.1
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(pt), math.sin(pt), math.cos(y), math.sin(y)
    R = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr], [-sp, cp * sr, cp * cr]])
    assert np.allclose(load_stl(p, rpy=(r, pt, y)), base @ R.T, rtol=0, atol=1e-14)
    # ASCII, and a file cut short
    a = str(tmp_path / "ascii.stl")
    open(a, "w").write("solid box\n facet normal 0 0 1\n  outer loop\n   vertex 0 0 0\n   vertex 1 0 0\n   vertex 0 1 0\n  endloop\n endfacet\nendsolid box\n")
    with pytest.raises(ValueError, match="ASCII"):
        load_stl(a)
    raw = open(p, "rb").read()
    open(p, "wb").write(raw[:-7])
    with pytest.raises(ValueError, match="do not hold"):
        load_stl(p)


def test_python_methods_exist():
    import bluerov2_amd
    for name in ("set_range_mesh", "range_mesh_info", "range_eval"):
        assert callable(getattr(bluerov2_amd.BatchSolver, name)), name
    import inspect
    assert "visits" in inspect.signature(bluerov2_amd.BatchSolver.range_eval).parameters
    for name in ("MeshInfo", "load_stl", "MESH_MAX_TRIANGLES"):
        assert name in bluerov2_amd.__all__, name
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "mesh_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
