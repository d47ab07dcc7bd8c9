"""The fleet in moving water (brov_vehicle_current_*, brov_vehicle_coriolis_*) without a GPU: the C ABI's symbols and declarations, the
argument checks that need no device, the Fleet methods' shape checks, the new kernel's resource report and the Makefile's gate."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
CURRENT = ["brov_vehicle_current_constant_host", "brov_vehicle_current_table_host", "brov_vehicle_current_gauss_markov_host",
           "brov_vehicle_current_off", "brov_vehicle_current_mode", "brov_vehicle_current_eval_host", "brov_vehicle_current_get_state_host",
           "brov_vehicle_current_set_state_host", "brov_vehicle_current_last_host"]
CORIOLIS = ["brov_vehicle_coriolis_set", "brov_vehicle_coriolis_off", "brov_vehicle_coriolis_terms", "brov_vehicle_coriolis_get",
            "brov_vehicle_coriolis_eval_host", "brov_vehicle_coriolis_last_host"]
SYMBOLS = CURRENT + CORIOLIS
METHODS = ("set_current", "current_off", "current_mode", "current", "current_state", "set_current_state", "current_last", "set_coriolis",
           "coriolis_off", "coriolis_terms", "coriolis_eval", "coriolis_last")


def _lib():
    import bluerov2_amd
    from bluerov2_amd.fleet import _fleet_lib
    bluerov2_amd.build_library()
    return _fleet_lib()


def _header():
    """bluerov2_nmpc.h as a compiler sees it for these families: with the file it includes for them, comments stripped"""
    inc = os.path.join(ROOT, "include")
    txt = open(os.path.join(inc, "bluerov2_nmpc.h")).read()
    assert txt.count('#include "bluerov2_nmpc_water.h"') == 1
    txt = txt.replace('#include "bluerov2_nmpc_water.h"', open(os.path.join(inc, "bluerov2_nmpc_water.h")).read())
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_library_exports_and_header_declares_every_new_symbol_with_its_signature():
    import bluerov2_amd
    bluerov2_amd.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and re.match(r"brov_vehicle_(current|coriolis)_", ln.split()[-1]))
    assert exported == set(SYMBOLS), sorted(exported ^ set(SYMBOLS))
    txt = _header()
    declared = set(re.findall(r"\b(brov_vehicle_(?:current|coriolis)_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(SYMBOLS), sorted(declared ^ set(SYMBOLS))
    flat = re.sub(r"\s+", " ", txt)
    for sig in ("int brov_vehicle_current_constant_host(brov_fleet* f, const double* v );",
                "int brov_vehicle_current_table_host(brov_fleet* f, const double* tab , int rows, const double* gain );",
                "int brov_vehicle_current_gauss_markov_host(brov_fleet* f, uint64_t seed, const double* mean , const double* mu , "
                "const double* amp , const double* lo , const double* hi , double step );",
                "int brov_vehicle_current_off(brov_fleet* f);", "int brov_vehicle_current_mode(const brov_fleet* f);",
                "int brov_vehicle_current_eval_host(brov_fleet* f, int64_t tick, double* v );",
                "int brov_vehicle_current_get_state_host(brov_fleet* f, double* v );",
                "int brov_vehicle_current_set_state_host(brov_fleet* f, const double* v );",
                "int brov_vehicle_current_last_host(brov_fleet* f, double* v );",
                "int brov_vehicle_coriolis_set(brov_fleet* f, int terms , double ka, double ma);",
                "int brov_vehicle_coriolis_off(brov_fleet* f);", "int brov_vehicle_coriolis_terms(const brov_fleet* f);",
                "int brov_vehicle_coriolis_get(const brov_fleet* f, int* terms, double* ka, double* ma);",
                "int brov_vehicle_coriolis_eval_host(brov_fleet* f, const double* x , const double* vc , double* c );",
                "int brov_vehicle_coriolis_last_host(brov_fleet* f, double* c );"):
        assert sig in flat, sig
    # the two paragraphs that called the fleet out of scope point to the families
    raw = open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read()
    assert "Out of scope and refused while a mode is in force" not in raw and "the water a fleet's vehicles move in is set with brov_vehicle_current_*" in raw
    assert "the stage of a fleet's vehicles is set with brov_vehicle_coriolis_*" in raw
    assert "brov_vehicle_current_*" in raw and "brov_vehicle_coriolis_*" in raw and "ONE body of water" in raw


def test_the_header_compiles_as_c_and_the_water_header_refuses_to_stand_alone(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "bluerov2_nmpc.h"\nint (*p)(brov_fleet*, int, double, double) = brov_vehicle_coriolis_set;\n'
                   'int (*q)(brov_fleet*, const double*, int, const double*) = brov_vehicle_current_table_host;\n')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(src)], check=True)
    alone = tmp_path / "a.c"
    alone.write_text('#include "bluerov2_nmpc_water.h"\n')
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-I", inc, str(alone)], capture_output=True, text=True)
    assert r.returncode != 0 and "include bluerov2_nmpc.h" in r.stderr


def test_null_handles_are_argument_errors_with_the_calls_own_name():
    L = _lib()
    dp = ctypes.POINTER(ctypes.c_double)
    buf = (ctypes.c_double * 12)()
    p = ctypes.cast(buf, dp)
    t, ka, ma = ctypes.c_int(0), ctypes.c_double(0), ctypes.c_double(0)
    calls = [("brov_vehicle_current_constant_host", (None, p)), ("brov_vehicle_current_table_host", (None, p, 1, None)),
             ("brov_vehicle_current_gauss_markov_host", (None, 1, p, p, p, None, None, 0.05)), ("brov_vehicle_current_off", (None,)),
             ("brov_vehicle_current_eval_host", (None, 0, p)), ("brov_vehicle_current_get_state_host", (None, p)),
             ("brov_vehicle_current_set_state_host", (None, p)), ("brov_vehicle_current_last_host", (None, p)),
             ("brov_vehicle_coriolis_set", (None, 1, 0.0, 1.0)), ("brov_vehicle_coriolis_off", (None,)),
             ("brov_vehicle_coriolis_get", (None, ctypes.byref(t), ctypes.byref(ka), ctypes.byref(ma))),
             ("brov_vehicle_coriolis_eval_host", (None, p, None, p)), ("brov_vehicle_coriolis_last_host", (None, p))]
    assert sorted(set(n for n, _ in calls) | {"brov_vehicle_current_mode", "brov_vehicle_coriolis_terms"}) == sorted(SYMBOLS)
    for name, args in calls:
        assert getattr(L, name)(*args) == ERR_ARG, (name, args)
        assert L.brov_fleet_last_error().decode().startswith(name + ":"), (name, L.brov_fleet_last_error())   # the text of THIS call
    assert L.brov_vehicle_current_mode(None) == 0       # BROV_CURRENT_OFF
    assert L.brov_vehicle_coriolis_terms(None) == 0


class _Down(Exception):
    pass


class _NoLib:
    """stands in for the library: a wrapper that reaches it has not rejected its arguments"""
    def __getattr__(self, name):
        def call(*a):
            raise _Down(name)
        return call


def _hollow_fleet(V=3, C=2):
    import bluerov2_amd
    f = object.__new__(bluerov2_amd.Fleet)
    f._L, f._h, f.V, f.C = _NoLib(), None, V, C
    return f


def test_fleet_methods_exist_and_reject_malformed_shapes_before_calling_down():
    import bluerov2_amd
    for name in METHODS:
        assert callable(getattr(bluerov2_amd.Fleet, name)), name
    f = _hollow_fleet()
    V = f.V
    gm = dict(mean=np.zeros(3), mu=0.5, amp=0.1)
    bad = [lambda: f.set_current(), lambda: f.set_current(constant=np.zeros(3), table=np.zeros((2, 3))),
           lambda: f.set_current(constant=np.zeros(3), gain=np.ones(V)), lambda: f.set_current(constant=np.zeros((V + 1, 3))),
           lambda: f.set_current(constant=np.zeros(4)), lambda: f.set_current(table=np.zeros((2, 4))), lambda: f.set_current(table=np.zeros(3)),
           lambda: f.set_current(table=np.zeros((0, 3))), lambda: f.set_current(table=np.zeros((2, 3)), gain=np.ones(V + 1)),
           lambda: f.set_current(gauss_markov=dict(mean=np.zeros(3), mu=0.5)), lambda: f.set_current(gauss_markov=dict(gm, sigma=1.0)),
           lambda: f.set_current(gauss_markov=dict(gm, mean=np.zeros((V, 2)))), lambda: f.set_current(gauss_markov=dict(gm, mu=np.zeros(2))),
           lambda: f.set_current(gauss_markov=dict(gm, lo=np.zeros(4))), lambda: f.set_current_state(np.zeros((V + 1, 3))),
           lambda: f.coriolis_eval(np.zeros((V, 11))), lambda: f.coriolis_eval(np.zeros((V + 1, 12))),
           lambda: f.coriolis_eval(np.zeros((V, 12)), vc=np.zeros((V, 2)))]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    # ... and well-formed arguments do go down, to the entry point meant
    for call, name in ((lambda: f.set_current(constant=np.zeros(3)), "brov_vehicle_current_constant_host"),
                       (lambda: f.set_current(table=np.zeros((2, 3)), gain=np.ones(V)), "brov_vehicle_current_table_host"),
                       (lambda: f.set_current(gauss_markov=gm), "brov_vehicle_current_gauss_markov_host"),
                       (lambda: f.set_current_state(np.zeros(3)), "brov_vehicle_current_set_state_host"),
                       (lambda: f.coriolis_eval(np.zeros((V, 12)), vc=np.zeros(3)), "brov_vehicle_coriolis_eval_host"),
                       (lambda: f.set_coriolis(3, ka=0.1), "brov_vehicle_coriolis_set")):
        with pytest.raises(_Down, match=name + "$"):
            call()


def test_the_new_kernel_uses_no_scratch_and_no_lds_and_the_makefile_gates_it():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "fleet_water_kernel.hip"], capture_output=True,
                         text=True, timeout=600).stdout
    rep = {}
    for ln in out.splitlines():
        m = re.match(r"Name: (\S+)", ln)
        if m and "fleet_plant_water_kernel" in m.group(1):
            rep[m.group(1)] = {k: int(v) for k, v in re.findall(r"\|([A-Za-z ]+): (\d+)", ln)}
    assert len(rep) == 4, sorted(rep)                     # <WR, CO>
    for name, r in rep.items():
        assert r["scratch"] == 0 and r["lds"] == 0 and r["AGPRs"] == 0 and r["VGPRs Spill"] == 0 and r["occ"] >= 2, (name, r)
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bfleet_water_kernel\.hip\b", mk, flags=re.M)
    rule = mk[mk.index("$(OUTDIR)/obj/fleet_water_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule and "fleet_plant_water_kernel" in rule
    for dep in ("fleet_plant_device.hpp", "current_gen.hpp", "plant_stages.hpp"):
        assert dep in rule, dep


def test_the_gather_is_shared_not_restated():
    """the winner / hold / status rule stands in one place, fleet_plant_device.hpp, and both kernel files reach it from there"""
    src = os.path.join(ROOT, "bluerov2_amd", "csrc")
    for name in ("fleet_kernel.hip", "fleet_water_kernel.hip"):
        txt = open(os.path.join(src, name)).read()
        assert '#include "fleet_plant_device.hpp"' in txt and "BROV_STATUS_NAN" not in txt and "A.winner[" not in txt, name
    shared = open(os.path.join(src, "fleet_plant_device.hpp")).read()
    assert "BROV_STATUS_NAN" in shared and "A.winner[" in shared
