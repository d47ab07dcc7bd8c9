"""The error-state filter (brov_eskf_*) without a GPU: the header's structure against the ctypes mirror, the exported symbols, the defaults, and the
refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import eskf_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SYMBOLS = ["brov_eskf_default_params", "brov_eskf_last_error", "brov_eskf_create", "brov_eskf_destroy", "brov_eskf_batch", "brov_eskf_reset",
           "brov_eskf_set_state_host", "brov_eskf_get_state_host", "brov_eskf_predict_host", "brov_eskf_predict_device", "brov_eskf_update_host",
           "brov_eskf_update_device", "brov_eskf_get_outputs_host", "brov_eskf_x_device", "brov_eskf_P_device", "brov_eskf_mpc_p_device",
           "brov_eskf_update_from_solver", "brov_eskf_apply_to_solver", "brov_eskf_get_inputs_host", "brov_eskf_last_update_seconds"]


def _lib():
    import bluerov2_amd
    from bluerov2_amd.eskf import _eskf_lib
    bluerov2_amd.build_library()
    return _eskf_lib()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc_eskf.h")).read(), flags=re.S)


def test_header_declares_and_library_exports_exactly_these_names():
    import bluerov2_amd
    bluerov2_amd.build_library()
    declared = set(re.findall(r"\b(brov_eskf_[a-z0-9_A-Z]+)\s*\(", _header()))
    assert declared == set(SYMBOLS), sorted(declared ^ set(SYMBOLS))
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("brov_eskf_"))
    assert exported == set(SYMBOLS), sorted(exported ^ set(SYMBOLS))
    main = open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read()
    assert '#include "bluerov2_nmpc_eskf.h"' in main and "brov_eskf_create" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)


def test_structure_fields_order_and_size_match_the_ctypes_mirror():
    import bluerov2_amd
    body = re.search(r"typedef struct brov_eskf_params \{(.*?)\} brov_eskf_params;", _header(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            fields.append((m.group(1), ctype, int(m.group(2) or 1)))
    mirror = [(n, "double" if (t is C.c_double or getattr(t, "_type_", None) is C.c_double) else "int32_t", getattr(t, "_length_", 1))
              for n, t in bluerov2_amd.EskfParams._fields_]
    assert fields == mirror, (fields, mirror)
    assert C.sizeof(bluerov2_amd.EskfParams) == 8 * sum(n for _, t, n in fields if t == "double") + 4 * sum(n for _, t, n in fields if t == "int32_t")
    assert [f for f, _ in X.PAR_FIELDS] == [n for n, _, _ in fields if n != "reserved"]
    assert callable(bluerov2_amd.BatchEskf.update_from_solver) and "BatchEskf" in bluerov2_amd.__all__ and "EskfParams" in bluerov2_amd.__all__


def test_defaults_are_the_reference_numbers():
    import bluerov2_amd
    _lib()
    p = bluerov2_amd.EskfParams.default()
    assert np.array_equal(X.par_vector(p), X.default_par_vector())
    assert p.dt == 1.0 / 50.0 and p.gps_dt == 1.0 / 30.0 and p.vel_inject == 2.0 and p.inject_bias_g == 0 and p.reserved == 0
    assert list(p.Q) == [0.001] * 21 and list(p.R12) == [0.01] * 3 + [0.02] * 3 + [0.0006] * 3 + [0.012] * 3
    e = bluerov2_amd.EkfParams.default()
    assert p.compensate_coef == e.compensate_coef and p.rotor_constant == e.rotor_constant and list(p.K) == list(e.K)


def test_refusals_come_before_any_device_is_touched():
    import bluerov2_amd
    L = _lib()
    h = C.c_void_p()

    def text():
        return L.brov_eskf_last_error().decode()
    assert L.brov_eskf_create(C.byref(h), 0, 0, None) == ERR_ARG and text().startswith("brov_eskf_create:") and "batch" in text() and not h
    assert L.brov_eskf_create(C.byref(h), 0, -3, None) == ERR_ARG
    for field, val in (("dt", 0.0), ("dt", -0.02), ("gps_dt", 0.0), ("dt", float("nan"))):
        p = bluerov2_amd.EskfParams.default()
        setattr(p, field, val)
        assert L.brov_eskf_create(C.byref(h), 0, 4, C.byref(p)) == ERR_ARG and "dt" in text() and not h, (field, val)
    for i, val in ((0, 0.0), (7, -1e-3), (11, float("nan"))):
        p = bluerov2_amd.EskfParams.default()
        p.R12[i] = val
        assert L.brov_eskf_create(C.byref(h), 0, 4, C.byref(p)) == ERR_ARG and f"R12[{i}]" in text() and not h
    # a quaternion that is not of unit length, or not finite: refused before the handle is looked at
    dp = C.POINTER(C.c_double)
    for q in ((0.0, 0.0, 0.0, 0.0), (1.0, 0.1, 0.0, 0.0), (float("nan"), 0.0, 0.0, 0.0), (float("inf"), 0.0, 0.0, 0.0)):
        x = np.zeros(22); x[6:10] = q
        assert L.brov_eskf_reset(None, x.ctypes.data_as(dp), None) == ERR_ARG and "quaternion" in text(), q
    x = np.zeros(22); x[6] = 1.0
    assert L.brov_eskf_reset(None, x.ctypes.data_as(dp), None) == ERR_ARG and "quaternion" not in text()      # a good state, no handle
    for name, args in (("brov_eskf_set_state_host", (None, None, None)), ("brov_eskf_get_state_host", (None, None, None)),
                       ("brov_eskf_predict_host", (None, None, None)), ("brov_eskf_update_host", (None,) * 7),
                       ("brov_eskf_get_outputs_host", (None,) * 5), ("brov_eskf_get_inputs_host", (None,) * 6),
                       ("brov_eskf_update_from_solver", (None, None, None)), ("brov_eskf_apply_to_solver", (None, None, None)),
                       ("brov_eskf_last_update_seconds", (None, None))):
        assert getattr(L, name)(*args) == ERR_ARG and text().startswith(name + ":"), (name, text())
    assert L.brov_eskf_batch(None) == 0 and L.brov_eskf_x_device(None) is None
