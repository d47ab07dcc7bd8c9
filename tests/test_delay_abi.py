"""The plant's delay stage (brov_delay_*) without a GPU: the C ABI's symbols and declarations, the argument checks that need no device, the
BatchSolver methods, the new kernels' resource report and the Makefile's gate."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SYMBOLS = ["brov_delay_set_host", "brov_delay_off", "brov_delay_enabled", "brov_delay_comp", "brov_delay_depth", "brov_delay_reset",
           "brov_delay_last_host", "brov_delay_queue_host", "brov_delay_predict_host", "brov_delay_predicted_host", "brov_delay_last_seconds"]
KERNELS = {"delay_shift_kernel": r"\d+delay_shift_kernelE", "delay_predict_kernel": r"\d+delay_predict_kernelE"}
PLANT_KERNEL_VGPRS = 150     # plant_kernel's registers: the predictor must stay at or below them, three waves per SIMD


def _lib():
    import bluerov2_amd
    from bluerov2_amd.solver import _load
    bluerov2_amd.build_library()
    return _load()


def test_header_declares_and_library_exports_exactly_the_eleven_names():
    import bluerov2_amd
    bluerov2_amd.build_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(brov_delay_[a-z0-9_]+)\s*\(", txt))
    assert len(SYMBOLS) == 11 and declared == set(SYMBOLS), sorted(declared ^ set(SYMBOLS))
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("brov_delay_"))
    assert exported == set(SYMBOLS), sorted(exported ^ set(SYMBOLS))
    assert re.search(r"#define\s+BROV_DELAY_MAX\s+8\b", txt)
    assert re.search(r"int\s+brov_delay_set_host\(brov_solver\* s, const int32_t\* delay\s*, int32_t comp, double dt_pred\s*,\s*"
                     r"int32_t observer_applied\);", txt)
    assert re.search(r"int\s+brov_delay_last_host\(brov_solver\* s, double\* u0_applied\s*, double\* thrust_applied\s*\);", txt)
    assert re.search(r"int\s+brov_delay_queue_host\(brov_solver\* s, double\* u0\s*\);", txt)
    assert re.search(r"int\s+brov_delay_predict_host\(brov_solver\* s, const double\* y, double\* xhat\);", txt)
    assert re.search(r"int\s+brov_delay_predicted_host\(brov_solver\* s, double\* xhat\s*\);", txt)
    assert re.search(r"int\s+brov_delay_last_seconds\(brov_solver\* s, double\* shift_s, double\* predict_s\);", txt)


def test_no_name_was_added_under_the_other_stages_prefixes():
    """the stage has its own prefix: the sets the other stages' tests pin stay as they are"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    for prefix in ("brov_thruster_", "brov_sensor_", "brov_current_", "brov_plant_wrench_"):
        assert not [n for n in re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", txt) if "delay" in n]


def test_null_handles_are_argument_errors_with_the_calls_own_name():
    L = _lib()
    buf = (ctypes.c_double * 12)()
    p = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))
    calls = [("brov_delay_set_host", (None, None, 0, 0.0, 0)), ("brov_delay_off", (None,)), ("brov_delay_reset", (None,)),
             ("brov_delay_last_host", (None, p, p)), ("brov_delay_queue_host", (None, p)), ("brov_delay_predict_host", (None, None, p)),
             ("brov_delay_predicted_host", (None, p)), ("brov_delay_last_seconds", (None, p, p))]
    for name, args in calls:
        assert getattr(L, name)(*args) == ERR_ARG, (name, args)
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())   # the text of THIS call
    assert L.brov_delay_enabled(None) == 0 and L.brov_delay_comp(None) == 0 and L.brov_delay_depth(None) == 0


def test_batch_solver_methods_exist():
    import bluerov2_amd
    for name in ("set_delay", "delay_off", "delay_enabled", "delay_last", "delay_queue", "delay_predict", "delay_predicted", "delay_reset",
                 "delay_last_seconds", "delay_comp", "delay_depth"):
        assert callable(getattr(bluerov2_amd.BatchSolver, name)), name


def test_new_kernels_use_no_scratch_no_lds_and_the_makefile_gates_them():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "delay_kernel.hip"], capture_output=True,
                         text=True, timeout=600).stdout
    rep = {}
    for ln in out.splitlines():
        m = re.match(r"Name: (\S+)", ln)
        if m:
            rep[m.group(1)] = {k: int(v) for k, v in re.findall(r"\|([A-Za-z ]+): (\d+)", ln)}
    for short, pat in KERNELS.items():
        hit = [r for m, r in rep.items() if re.search(pat, m)]
        assert len(hit) == 1, (short, sorted(rep))
        print(short, hit[0])
        assert hit[0]["scratch"] == 0 and hit[0]["lds"] == 0, (short, hit[0])
        assert hit[0]["occ"] >= 2, (short, hit[0])
    pred = [r for m, r in rep.items() if re.search(KERNELS["delay_predict_kernel"], m)][0]
    assert pred["VGPRs"] <= PLANT_KERNEL_VGPRS and pred["occ"] >= 3, pred
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "delay_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/delay_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    assert "delay_shift_kernel" in rule and "delay_predict_kernel" in rule
