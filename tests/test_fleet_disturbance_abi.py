"""The fleet under disturbance (brov_vehicle_*, brov_closed_loop_fleet_dob) without a GPU: the C ABI's symbols and declarations, the
argument checks that need no device, the Fleet methods, the new kernels' resource report and the Makefile's gate."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SYMBOLS = ["brov_vehicle_wrench_constant_host", "brov_vehicle_wrench_periodic", "brov_vehicle_wrench_table_host", "brov_vehicle_wrench_off",
           "brov_vehicle_wrench_mode", "brov_vehicle_wrench_seek", "brov_vehicle_wrench_tick", "brov_vehicle_wrench_eval_host",
           "brov_vehicle_observe", "brov_vehicle_apply_estimate", "brov_closed_loop_fleet_dob"]
KERNELS = ("fleet_plant_wrench_kernel", "fleet_observe_inputs_kernel", "fleet_apply_kernel")


def _lib():
    import bluerov2_amd
    from bluerov2_amd.fleet import _fleet_lib
    bluerov2_amd.build_library()
    return _fleet_lib()


def test_library_exports_and_header_declares_every_new_symbol():
    import bluerov2_amd
    bluerov2_amd.build_library()
    lib = ctypes.CDLL(bluerov2_amd.library_path())
    missing = [n for n in SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(brov_vehicle_[a-z0-9_]+|brov_closed_loop_fleet_dob)\s*\(", txt))
    assert declared == set(SYMBOLS), sorted(declared ^ set(SYMBOLS))
    assert re.search(r"int\s+brov_closed_loop_fleet_dob\(brov_fleet\* f, brov_ekf\* e\s*, int ticks, double t0, double dt_ref, double dt_node,\s*"
                     r"double dt, int substeps, double\* u_log, double\* x_log, int32_t\* st_log, int32_t\* win_log,\s*"
                     r"double\* w_log\s*, double\* est_log\s*\);", txt)
    assert re.search(r"int64_t\s+brov_vehicle_wrench_tick\(const brov_fleet\* f\);", txt)


def test_null_arguments_are_argument_errors_with_a_text():
    L = _lib()
    dp = ctypes.POINTER(ctypes.c_double)
    six = (ctypes.c_double * 6)()
    h = ctypes.c_void_p(0x1234)           # never dereferenced: every call below fails on its NULL argument first
    p6 = ctypes.cast(six, dp)
    calls = [("brov_vehicle_wrench_constant_host", (None, p6)), ("brov_vehicle_wrench_constant_host", (h, None)),
             ("brov_vehicle_wrench_periodic", (None, 1, 6.0, 0.0, 0.125, 3.0)),
             ("brov_vehicle_wrench_table_host", (None, p6, 1, None)), ("brov_vehicle_wrench_table_host", (h, None, 1, None)),
             ("brov_vehicle_wrench_off", (None,)), ("brov_vehicle_wrench_seek", (None, 3)),
             ("brov_vehicle_wrench_eval_host", (None, 0, p6)), ("brov_vehicle_wrench_eval_host", (h, 0, None)),
             ("brov_vehicle_observe", (None, h, 0.05, None)), ("brov_vehicle_observe", (h, None, 0.05, None)),
             ("brov_vehicle_apply_estimate", (None, h, None)), ("brov_vehicle_apply_estimate", (h, None, None)),
             ("brov_closed_loop_fleet_dob", (None, None, 1, 0.0, 0.05, 0.05, 0.05, 1, None, None, None, None, None, None))]
    for name, args in calls:
        assert getattr(L, name)(*args) == ERR_ARG, (name, args)
        assert L.brov_fleet_last_error().decode().startswith(name + ":"), (name, L.brov_fleet_last_error())   # the text of THIS call
    assert L.brov_vehicle_wrench_mode(None) == 0
    assert L.brov_vehicle_wrench_tick(None) == 0


def test_fleet_methods_exist():
    import bluerov2_amd
    for name in ("set_wrench", "wrench_off", "wrench_mode", "wrench", "wrench_seek", "wrench_tick", "observe", "apply_estimate",
                 "closed_loop_dob"):
        assert callable(getattr(bluerov2_amd.Fleet, name)), name


def test_new_kernels_use_no_scratch_and_no_lds_and_the_makefile_gates_them():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "fleet_kernel.hip"], capture_output=True,
                         text=True, timeout=600).stdout
    rep = {}
    for ln in out.splitlines():
        m = re.match(r"Name: (\S+)", ln)
        if m:
            rep[m.group(1)] = {k: int(v) for k, v in re.findall(r"\|([A-Za-z ]+): (\d+)", ln)}
    names = {short: r for mangled, r in rep.items() for short in KERNELS if re.search(r"\d+%sE" % short, mangled)}
    assert set(names) == set(KERNELS), sorted(rep)
    for short, r in names.items():
        assert r["scratch"] == 0 and r["lds"] == 0, (short, r)
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("$(OUTDIR)/obj/fleet_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    for k in KERNELS:
        assert k in rule, k
