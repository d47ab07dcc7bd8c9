"""The plant's thruster stage (brov_thruster_*) without a GPU: the C ABI's symbols and declarations, the argument checks that need no
device, the default propulsion matrix, the BatchSolver methods, the new kernels' resource report and the Makefile's gate, the fixture of the
reference's settings, and the numpy restatement against answers worked by hand."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np

from thruster_restatement import ThrusterRestatement, K_MODEL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SYMBOLS = ["brov_thruster_default_matrix", "brov_thruster_set_host", "brov_thruster_off", "brov_thruster_enabled", "brov_thruster_eval_host",
           "brov_thruster_last_host", "brov_thruster_get_stats_host", "brov_thruster_reset_stats", "brov_thruster_last_seconds"]
KERNELS = {"thruster_eval_kernel": r"\d+thruster_eval_kernelE", "plant_thruster_kernel<NoWorldWrench>": r"\d+plant_thruster_kernelINS_\d+NoWorldWrenchE",
           "plant_thruster_kernel<WorldWrench>": r"\d+plant_thruster_kernelINS_\d+WorldWrenchE"}


def _lib():
    import bluerov2_amd
    from bluerov2_amd.solver import _load
    bluerov2_amd.build_library()
    return _load()


def test_header_declares_and_library_exports_exactly_the_nine_names():
    import bluerov2_amd
    bluerov2_amd.build_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(brov_thruster_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(SYMBOLS), sorted(declared ^ set(SYMBOLS))
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("brov_thruster_"))
    assert exported == set(SYMBOLS), sorted(exported ^ set(SYMBOLS))
    assert re.search(r"int\s+brov_thruster_set_host\(brov_solver\* s, const double\* K\s*, const double\* lo\s*,\s*const double\* hi\s*, "
                     r"const double\* gain\s*,\s*const double\* bias\s*, const int64_t\* onset\s*\);", txt)
    assert re.search(r"int\s+brov_thruster_eval_host\(brov_solver\* s, int64_t tick, const double\* commanded\s*, double\* applied\s*, "
                     r"double\* wrench\s*\);", txt)
    assert re.search(r"int\s+brov_thruster_get_stats_host\(brov_solver\* s, int32_t\* clip_ticks\s*, double\* lost_sq\s*, int64_t\* steps\s*\);", txt)
    assert re.search(r"void\s+brov_thruster_default_matrix\(double K\[36\]\);", txt)


def test_null_handles_are_argument_errors_with_the_calls_own_name():
    L = _lib()
    six = (ctypes.c_double * 6)()
    p6 = ctypes.cast(six, ctypes.POINTER(ctypes.c_double))
    sec = ctypes.c_double(0.0)
    calls = [("brov_thruster_set_host", (None, None, None, None, None, None, None)), ("brov_thruster_off", (None,)),
             ("brov_thruster_eval_host", (None, 0, p6, p6, p6)), ("brov_thruster_last_host", (None, p6)),
             ("brov_thruster_get_stats_host", (None, None, None, None)), ("brov_thruster_reset_stats", (None,)),
             ("brov_thruster_last_seconds", (None, ctypes.byref(sec)))]
    for name, args in calls:
        assert getattr(L, name)(*args) == ERR_ARG, (name, args)
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())   # the text of THIS call
    assert L.brov_thruster_enabled(None) == 0


def test_default_matrix_is_the_models():
    L = _lib()
    K = np.full((6, 6), np.nan)
    L.brov_thruster_default_matrix(K.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    # the reference's bluerov2.py:95-100, written out
    expect = np.array([[0.707, 0.707, -0.707, -0.707, 0, 0],
                       [0.707, -0.707, 0.707, -0.707, 0, 0],
                       [0, 0, 0, 0, 1, 1],
                       [0, 0, 0, 0, 0, 0],
                       [0, 0, 0, 0, 0, 0],
                       [0.167, -0.167, -0.175, 0.175, 0, 0]])
    assert np.array_equal(K, expect) and np.array_equal(K_MODEL, expect)
    import bluerov2_amd
    assert np.array_equal(bluerov2_amd.BatchSolver.thruster_matrix(), expect)
    L.brov_thruster_default_matrix(None)   # nothing to write to: a no-op


def test_batch_solver_methods_exist():
    import bluerov2_amd
    for name in ("set_thrusters", "thrusters_off", "thrusters_enabled", "thruster_eval", "thruster_last", "thruster_stats", "thruster_reset_stats",
                 "thruster_last_seconds", "thruster_matrix"):
        assert callable(getattr(bluerov2_amd.BatchSolver, name)), name


def test_new_kernels_use_no_scratch_and_the_makefile_gates_them():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "plant_wrench.hip"], capture_output=True,
                         text=True, timeout=600).stdout
    rep = {}
    for ln in out.splitlines():
        m = re.match(r"Name: (\S+)", ln)
        if m:
            rep[m.group(1)] = {k: int(v) for k, v in re.findall(r"\|([A-Za-z ]+): (\d+)", ln)}
    for short, pat in KERNELS.items():
        hit = [r for m, r in rep.items() if re.search(pat, m)]
        assert len(hit) == 1, (short, sorted(rep))
        assert hit[0]["scratch"] == 0 and hit[0]["lds"] == 0, (short, hit[0])
        assert hit[0]["VGPRs"] <= 256 and hit[0]["occ"] >= 2, (short, hit[0])
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "plant_wrench.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/plant_wrench.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    assert "plant_thruster_kernel" in rule and "thruster_eval_kernel" in rule


def test_fixture_holds_the_reference_settings():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "thruster_tam.json")))
    tam = np.array(g["tam"])
    assert tam.shape == (6, 6) and g["max_thrust"] == 1540.0 and g["proportional_gain"] == 0.026546960744430276
    assert "TAM.yaml" in g["source"] and "thruster_manager.yaml:7" in g["source"]
    # the matrix the model rounds to three digits: rows 0, 1, 2, 5 agree with the model's to 1e-3, rows 3 and 4 carry the moments it drops
    assert np.abs(tam[[0, 1, 2, 5]] - K_MODEL[[0, 1, 2, 5]]).max() < 1e-3 and np.abs(tam[3:5]).max() > 0.1
    # one axis at its bound of 50 already asks a horizontal thruster for more than the manager delivers
    assert 50.0 / g["proportional_gain"] > g["max_thrust"]


def test_restatement_has_the_answers_worked_by_hand():
    """Three thrusters commanded, thruster 1 below its limit; instance 0 ahead of its onset tick, instance 1 past it with gain 0.5 and bias 8 on
    thruster 0.  Every number is a small dyadic rational, so each rounded operation is exact and the literals are the hand computation."""
    K = [[1, 1, -1, -1, 0, 0], [1, -1, 1, -1, 0, 0], [0, 0, 0, 0, 1, 1], [0.5, 0, 0, 0, -0.25, 0.25], [0, 0, 0, 0, 0, 0], [0.25, -0.25, -0.5, 0.5, 0, 0]]
    r = ThrusterRestatement(2, K=K, lo=-100.0, hi=100.0, gain=[0.5, 1, 1, 1, 1, 1], bias=[8.0, 0, 0, 0, 0, 0], onset=[5, 0])
    t = np.tile([40.0, -250.0, 64.0, 0.0, 0.0, 0.0], (2, 1))
    a, g = r.stage(3, t)
    # c = (40, -100, 64, 0, 0, 0) for both; instance 1: a0 = 0.5 * 40 + 8 = 28
    assert np.array_equal(a, [[40.0, -100.0, 64.0, 0.0, 0.0, 0.0], [28.0, -100.0, 64.0, 0.0, 0.0, 0.0]])
    # instance 0: X = 40 - 100 - 64 = -124, Y = 40 + 100 + 64 = 204, K = 20, N = 10 + 25 - 32 = 3;  instance 1: -136, 192, 14, 7 + 25 - 32 = 0
    assert np.array_equal(g, [[-124.0, 204.0, 0.0, 20.0, 0.0, 3.0], [-136.0, 192.0, 0.0, 14.0, 0.0, 0.0]])
    assert r.steps == 0 and not r.clip_ticks.any() and not r.lost_sq.any()            # evaluation touches no statistic
    a2, g2 = r.step(3, t)
    assert np.array_equal(a2, a) and np.array_equal(g2, g)
    assert np.array_equal(r.clip_ticks, [[0, 1, 0, 0, 0, 0]] * 2)
    assert np.array_equal(r.lost_sq, [150.0 ** 2, 12.0 ** 2 + 150.0 ** 2]) and np.array_equal(r.lost_sq, [22500.0, 22644.0])
    assert np.array_equal(r.last, a) and r.steps == 1
    r.step(5, t)                                                                  # now both are past their onset
    assert np.array_equal(r.last, [[28.0, -100.0, 64.0, 0.0, 0.0, 0.0]] * 2)
    assert np.array_equal(r.clip_ticks, [[0, 2, 0, 0, 0, 0]] * 2) and np.array_equal(r.lost_sq, [22500.0 + 22644.0, 2 * 22644.0]) and r.steps == 2
    # a NaN command passes through the limits; a command exactly on a limit is not clipped
    a3, _ = r.stage(0, np.array([[np.nan, -100.0, 100.0, 0.0, -0.0, 0.0]] * 2))
    assert np.isnan(a3[:, 0]).all() and np.array_equal(a3[0, 1:], [-100.0, 100.0, 0.0, -0.0, 0.0]) and np.signbit(a3[0, 4])
