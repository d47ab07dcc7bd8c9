"""The range stage (brov_range_*), the inspection controller (brov_inspect_*) and their loop without a GPU: the C ABI's symbols and
declarations (include/bluerov2_nmpc_inspect.h), the structures against their ctypes and numpy mirrors with the defaults, the refusals that need
no device, the Python methods."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
RANGE = ["brov_range_default_params", "brov_range_focal", "brov_range_set_scene_host", "brov_range_set_host", "brov_range_eval_host",
         "brov_range_last_seconds"]
INSPECT = ["brov_inspect_default_params", "brov_inspect_set_host", "brov_inspect_off", "brov_inspect_enabled", "brov_inspect_reset",
           "brov_inspect_eval_host", "brov_inspect_get_state_host", "brov_inspect_get_stats_host", "brov_inspect_reset_stats",
           "brov_inspect_last_seconds", "brov_inspect_step"]
LOOP = ["brov_closed_loop_inspect"]


def _lib():
    import bluerov2_amd
    from bluerov2_amd.solver import _load
    bluerov2_amd.build_library()
    return _load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc_inspect.h")).read(), flags=re.S)


def test_header_declares_and_library_exports_the_new_names():
    import bluerov2_amd
    bluerov2_amd.build_library()
    declared = set(re.findall(r"\b(brov_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(RANGE) | set(INSPECT) | set(LOOP), sorted(declared ^ (set(RANGE) | set(INSPECT) | set(LOOP)))
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split())
    assert declared <= exported, sorted(declared - exported)
    assert set(n for n in exported if n.startswith("brov_range_")) == set(RANGE)
    assert set(n for n in exported if n.startswith("brov_inspect_")) == set(INSPECT)
    main = open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read()
    assert main.count('#include "bluerov2_nmpc_inspect.h"') == 1
    assert main.index('#include "bluerov2_nmpc_inspect.h"') > main.index('#include "bluerov2_nmpc_imu.h"')
    assert "brov_inspect_set_host" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    h = _header()
    assert "BROV_RANGE_MAX_BOXES 8" in h and "BROV_INSPECT_SHARED_PID 1" in h and "BROV_INSPECT_FLOAT_YAW 2" in h


def _fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    out = []
    for d in body.split(";"):
        if d.strip():
            t, n = d.split()
            m = re.match(r"(\w+)\[(\d+)\]$", n)
            out.append((t, m.group(1), int(m.group(2))) if m else (t, n, 1))
    return out


def _ctypes_fields(cls):
    names = {C.c_double: "double", C.c_int32: "int32_t", C.c_uint64: "uint64_t", C.c_int64: "int64_t"}
    return [(names[getattr(t, "_type_", t)] if hasattr(t, "_length_") else names[t], n, getattr(t, "_length_", 1)) for n, t in cls._fields_]


def _dtype_fields(dt):
    names = {"float64": "double", "int32": "int32_t", "int64": "int64_t"}
    return [(names[dt.fields[n][0].base.name], n, int(np.prod(dt.fields[n][0].shape, dtype=int))) for n in dt.names]


def test_structures_match_their_mirrors_with_defaults():
    import bluerov2_amd
    from bluerov2_amd import inspect as I
    assert _fields("brov_range_params") == _ctypes_fields(bluerov2_amd.RangeParams)
    assert _fields("brov_inspect_params") == _ctypes_fields(bluerov2_amd.InspectParams)
    assert _fields("brov_inspect_state") == _dtype_fields(bluerov2_amd.INSPECT_STATE_DTYPE)
    assert _fields("brov_inspect_stats") == _dtype_fields(bluerov2_amd.INSPECT_STATS_DTYPE)
    assert C.sizeof(bluerov2_amd.RangeParams) == 80 and C.sizeof(bluerov2_amd.InspectParams) == 208
    assert bluerov2_amd.INSPECT_STATE_DTYPE.itemsize == 128 and bluerov2_amd.INSPECT_STATS_DTYPE.itemsize == 56
    assert (bluerov2_amd.RANGE_MAX_BOXES, bluerov2_amd.INSPECT_SHARED_PID, bluerov2_amd.INSPECT_FLOAT_YAW) == (8, 1, 2)
    L = _lib()
    p = bluerov2_amd.RangeParams()
    L.brov_range_default_params(C.byref(p))
    assert bytes(p) == bytes(I.default_range_params())
    assert (p.roi, p.cx, p.cy, tuple(p.mount), p.near, p.far, p.seed) == (40, 0.0, 0.0, (0.0, 0.0, 0.0), 0.1, 100.0, 0)
    assert p.f == L.brov_range_focal(1280.0, 85.2 * math.pi / 180.0) == 1280.0 / (2.0 * math.tan(85.2 * math.pi / 180.0 / 2.0))
    c = bluerov2_amd.InspectParams()
    L.brov_inspect_default_params(C.byref(c))
    assert bytes(c) == bytes(I.default_inspect_params())
    assert (c.dt, c.safety_dis, c.buffer, c.sway, c.sway_slow, c.surge_search, c.z0, c.yaw0) == (0.05, 1.79, 0.5, -4.0, -2.0, 1.0, -34.5, 0.5 * math.pi)
    assert (c.lost, c.yaw_tol, c.yaw_home_tol, c.z_tol, c.height_tol, c.t_hold, c.flags) == (0.1, 0.1, 0.2, 0.25, 0.1, 1.0, 3)
    assert c.dz_round == 1.79 * math.tan(32 * math.pi / 180) * 2 and c.z_goal == c.z0 + c.dz_round
    assert list(c.gains) == [5, 0, 0, 5, 0, 0, 7, 0.08, 0]


def test_null_handles_are_argument_errors_with_the_calls_own_name():
    L = _lib()
    sec = C.c_double(0.0)
    calls = [("brov_range_set_scene_host", (None, 0, None, None)), ("brov_range_set_host", (None, None, None)),
             ("brov_range_eval_host", (None, 0) + (None,) * 5), ("brov_range_last_seconds", (None, C.byref(sec))),
             ("brov_inspect_set_host", (None, None)), ("brov_inspect_off", (None,)), ("brov_inspect_reset", (None,)),
             ("brov_inspect_eval_host", (None,) * 8), ("brov_inspect_get_state_host", (None,) * 3), ("brov_inspect_get_stats_host", (None, None)),
             ("brov_inspect_reset_stats", (None,)), ("brov_inspect_last_seconds", (None, C.byref(sec))), ("brov_inspect_step", (None, None)),
             ("brov_closed_loop_inspect", (None, 1, 0.05, 1, None, None, None, None))]
    for name, args in calls:
        assert getattr(L, name)(*args) == ERR_ARG, name
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())
    assert L.brov_inspect_enabled(None) == 0
    L.brov_range_default_params(None); L.brov_inspect_default_params(None)      # tolerated


def test_refusals_come_with_their_text_and_before_any_device_is_touched():
    """Each refusal of the three setters, of a step and of a plant step with another dt.  A solver handle needs a device, the checks need none:
    the host side (inspect_source.hpp, header only) is compiled into a stand-alone host program whose call context counts the waits and whose
    launchers abort (tests/inspect_refusals_main.cpp)."""
    src = os.path.join(ROOT, "tests", "inspect_refusals_main.cpp")
    exe = os.path.join(ROOT, "bluerov2_amd", "lib", "inspect_refusals")
    import bluerov2_amd
    bluerov2_amd.build_library()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", f"-I{ROOT}/include", f"-I{ROOT}/bluerov2_amd/csrc", src, "-o", exe,
                    "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(ln.split(" => ", 1) for ln in out.stdout.splitlines() if " => " in ln)
    want = {"9 boxes": "0 ... BROV_RANGE_MAX_BOXES", "-1 boxes": "0 ... BROV_RANGE_MAX_BOXES", "lo > hi": "lo > hi", "lo NaN": "not finite",
            "hi inf": "not finite", "null boxes": "null argument",
            "roi odd": "roi must be even", "roi 0": "roi must be even", "roi 66": "roi must be even", "f = 0": "f must be positive",
            "f < 0": "f must be positive", "f NaN": "not finite", "cx inf": "not finite", "mount NaN": "not finite", "near = far": "near must be below far",
            "near > far": "near must be below far", "sigma < 0": "sigma must be >= 0", "sigma NaN": "sigma must be >= 0", "null camera": "null argument",
            "dt = 0": "dt must be positive", "dt NaN": "not finite", "gain inf": "not finite", "z_goal NaN": "not finite", "flag 4": "unknown flag",
            "null controller": "null argument",
            "controller off": "controller is off", "no box": "no box", "comp > 0": "comp > 0", "index 2^24": "[0, 2^24)", "dt != dt": "dt is not its period"}
    for case, text in want.items():
        assert case in lines and lines[case].startswith("-1 brov_inspect_test: ") and text in lines[case], (case, lines.get(case))
    assert lines["waits"] == "0" and lines["allocations"] == "0"


def test_python_methods_exist():
    import bluerov2_amd
    for name in ("set_range_scene", "set_range", "range_eval", "range_last_seconds", "set_inspect", "inspect_off", "inspect_enabled", "inspect_reset",
                 "inspect_eval", "inspect_state", "inspect_stats", "inspect_reset_stats", "inspect_last_seconds", "inspect_step", "closed_loop_inspect"):
        assert callable(getattr(bluerov2_amd.BatchSolver, name)), name
    for name in ("RangeParams", "InspectParams", "INSPECT_STATE_DTYPE", "INSPECT_STATS_DTYPE", "INSPECT_SHARED_PID", "INSPECT_FLOAT_YAW"):
        assert name in bluerov2_amd.__all__, name
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "inspect_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
