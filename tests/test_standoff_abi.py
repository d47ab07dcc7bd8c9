"""The stand-off term of the fleet loop (brov_standoff_*, include/bluerov2_nmpc_standoff.h) without a GPU: the library exports exactly the
declared family, the header's declarations are what the ctypes mirror of bluerov2_amd/fleet.py binds, and a null handle is an argument error
whose text begins with the call's name."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SYMBOLS = ["brov_standoff_set", "brov_standoff_off", "brov_standoff_enabled", "brov_standoff_eval_device", "brov_standoff_eval_host",
           "brov_standoff_get_stats_host", "brov_standoff_last_seconds"]
CTYPES = {"brov_fleet*": C.c_void_p, "const brov_fleet*": C.c_void_p, "const brov_result*": C.c_void_p, "brov_result*": C.c_void_p, "void*": C.c_void_p,
          "double": C.c_double, "int": C.c_int, "double*": C.POINTER(C.c_double), "const double*": C.POINTER(C.c_double),
          "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64)}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc_standoff.h")).read(), flags=re.S)


def test_library_exports_and_header_declares_exactly_the_standoff_family():
    import bluerov2_amd
    bluerov2_amd.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split())
    assert sorted(n for n in exported if n.startswith("brov_standoff_")) == sorted(SYMBOLS)
    assert sorted(set(re.findall(r"\b(brov_standoff_[a-z0-9_]+)\s*\(", _header()))) == sorted(SYMBOLS)
    main = open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read()
    assert main.index('#include "bluerov2_nmpc_mesh.h"') < main.index('#include "bluerov2_nmpc_standoff.h"')
    assert "brov_standoff_set" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)      # declared in its own header only


def test_the_declarations_match_the_ctypes_mirror():
    from bluerov2_amd.fleet import STANDOFF_PROTOS, _fleet_lib
    assert sorted(STANDOFF_PROTOS) == sorted(SYMBOLS)
    decl = dict(re.findall(r"int\s+(brov_standoff_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header()))
    assert sorted(decl) == sorted(SYMBOLS)
    # two doubles in a row are a mirror's easiest mistake: the parameter names are part of what is held
    assert re.sub(r"\s+", " ", decl["brov_standoff_set"]) == "brov_fleet* f, double radius, double weight, double reach, int first"
    for name, params in decl.items():
        types = [re.sub(r"\s+", " ", p).strip().rsplit(" ", 1)[0] for p in params.split(",")]
        if name.endswith("_device"):                               # device addresses travel as integers: every pointer is a void* there
            assert all(t.endswith("*") and t in CTYPES for t in types) and STANDOFF_PROTOS[name] == [C.c_void_p] * len(types), (name, types)
        else:
            assert [CTYPES[t] for t in types] == STANDOFF_PROTOS[name], (name, types)
    L = _fleet_lib()
    for name in SYMBOLS:
        fn = getattr(L, name)
        assert fn.argtypes == STANDOFF_PROTOS[name] and fn.restype is C.c_int, name


def test_null_arguments_are_argument_errors_named_after_the_call():
    import bluerov2_amd
    from bluerov2_amd.fleet import _fleet_lib
    L = _fleet_lib()
    d = (C.c_double * 4)()
    calls = {
        "brov_standoff_set": lambda: L.brov_standoff_set(None, 1.0, 1.0, 1.0, 1),
        "brov_standoff_off": lambda: L.brov_standoff_off(None),
        "brov_standoff_eval_device": lambda: L.brov_standoff_eval_device(None, None, None, None, None, None, None),
        "brov_standoff_eval_host": lambda: L.brov_standoff_eval_host(None, None, d, None, None),
        "brov_standoff_get_stats_host": lambda: L.brov_standoff_get_stats_host(None, None, None, None),
        "brov_standoff_last_seconds": lambda: L.brov_standoff_last_seconds(None, d),
    }
    for name, call in calls.items():
        assert call() == ERR_ARG, name
        assert L.brov_fleet_last_error().decode() == name + (": null argument" if name != "brov_standoff_last_seconds" else ": no distance kernel yet")
    assert L.brov_standoff_enabled(None) == 0
    for name in ("set_standoff", "standoff_off", "standoff_enabled", "standoff_eval", "standoff_stats", "standoff_seconds"):
        assert callable(getattr(bluerov2_amd.Fleet, name))
