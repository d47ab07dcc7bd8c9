"""The fleet planning loop (brov_fleet_*, brov_closed_loop_fleet) without a GPU: the C ABI's symbols, the argument check that needs no
device, hand-written answers of the numpy restatement the kernels are held to, and the kernels' resource report."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fleet_restatement as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BROV_FLEET_SYMBOLS = ["brov_fleet_last_error", "brov_fleet_create", "brov_fleet_destroy", "brov_fleet_vehicles", "brov_fleet_candidates",
                      "brov_fleet_reset", "brov_fleet_set_state_host", "brov_fleet_get_state_host", "brov_fleet_set_plant_params_host",
                      "brov_fleet_select_device", "brov_fleet_select_host", "brov_fleet_step", "brov_fleet_get_last_host",
                      "brov_fleet_last_seconds"]


def _recs(cost, status=None, u0=None):
    cost = np.asarray(cost, dtype=np.float64)
    r = np.zeros(cost.size, dtype=FR.RESULT_DTYPE)
    r["cost"] = cost
    r["status"] = 0 if status is None else status
    r["u0"] = np.arange(cost.size * 4).reshape(-1, 4) + 1.0 if u0 is None else u0
    r["kkt"] = np.arange(cost.size) * 0.5
    return r


def test_library_exports_every_fleet_symbol():
    import bluerov2_amd
    bluerov2_amd.build_library()
    lib = ctypes.CDLL(bluerov2_amd.library_path())
    missing = [n for n in BROV_FLEET_SYMBOLS + ["brov_closed_loop_fleet"] if not hasattr(lib, n)]
    assert not missing, missing
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(brov_fleet_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(BROV_FLEET_SYMBOLS)
    assert re.search(r"int\s+brov_closed_loop_fleet\(brov_fleet\* f, int ticks, double t0, double dt_ref, double dt_node, double dt, int substeps,\s*"
                     r"double\* u_log, double\* x_log, int32_t\* st_log, int32_t\* win_log\);", txt)


def test_create_on_a_null_solver_is_an_argument_error():
    import bluerov2_amd
    from bluerov2_amd.fleet import _fleet_lib
    bluerov2_amd.build_library()
    L = _fleet_lib()
    h = ctypes.c_void_p(0x1234)
    assert L.brov_fleet_create(ctypes.byref(h), None, 3) == -1     # BROV_ERR_ARG
    assert L.brov_fleet_last_error().decode()
    assert L.brov_fleet_create(None, None, 3) == -1
    assert L.brov_fleet_vehicles(None) == 0 and L.brov_fleet_candidates(None) == 0
    L.brov_fleet_destroy(None)
    assert L.brov_fleet_step(None, None, 0.05, 1, None) == -1
    assert L.brov_closed_loop_fleet(None, 1, 0.0, 0.05, 0.05, 0.05, 1, None, None, None, None) == -1
    assert bluerov2_amd.Fleet is bluerov2_amd.fleet.Fleet
    for name in ("reset", "set_state", "state", "set_plant_params", "select", "select_device", "step", "last", "closed_loop", "last_seconds", "close"):
        assert callable(getattr(bluerov2_amd.Fleet, name))


def test_restatement_record_layout():
    import bluerov2_amd
    assert FR.RESULT_DTYPE == bluerov2_amd.RESULT_DTYPE


def test_restatement_lowest_cost_and_ties():
    # vehicle 0: a plain minimum; vehicle 1: a tie of three, the lowest index wins; vehicle 2: every cost equal; vehicle 3: -0.0 == 0.0
    r = _recs([5, 2, 9, 7,   3, 1, 1, 1,   4, 4, 4, 4,   0.0, -0.0, 0.0, 1])
    w, wr = FR.select(r, 4, 4)
    assert list(w) == [1, 1, 0, 0]
    assert wr.tobytes() == r[[1, 5, 8, 12]].tobytes()
    # costs of mixed sign: the most negative wins, not the smallest magnitude
    w, _ = FR.select(_recs([1, -3, 0.5, -2.5]), 1, 4)
    assert list(w) == [1]


def test_restatement_all_failed_and_failed_candidate_with_the_lowest_cost():
    r = _recs([1, 2, 3,   -100, 5, 6,   7, 8, 9], status=[4, 2, 1,   4, 0, 0,   0, 3, 0])
    w, wr = FR.select(r, 3, 3)
    assert list(w) == [-1, 1, 0]                               # the failed candidate's -100 does not win
    assert wr[0].tobytes() == bytes(104) and wr[1].tobytes() == r[4].tobytes() and wr[2].tobytes() == r[6].tobytes()
    w, u, st = FR.apply(r, 3, 3, u_hold=np.full((3, 4), 0.25))
    assert list(st) == [4, 0, 0]                               # without a winner: candidate 0's status
    assert list(u[0]) == [0.25] * 4 and list(u[1]) == list(r["u0"][4]) and list(u[2]) == list(r["u0"][6])


def test_restatement_non_finite_costs_never_win():
    r = _recs([np.nan, np.inf, -np.inf, 8.0,   np.nan, -np.inf, np.inf, np.nan])
    w, wr = FR.select(r, 2, 4)
    assert list(w) == [3, -1]
    assert wr[1].tobytes() == bytes(104)
    # success with a NaN cost on candidate 0 and nobody else eligible: the status is STATUS_NAN, the input is held
    r = _recs([np.nan, 3.0, -np.inf], status=[0, 2, 0])
    w, u, st = FR.apply(r, 1, 3, u_hold=np.zeros((1, 4)))
    assert list(w) == [-1] and list(st) == [FR.STATUS_NAN] and not u.any()
    # ... while a failed candidate 0 reports its own status
    r["status"][0] = 3
    assert list(FR.apply(r, 1, 3, np.zeros((1, 4)))[2]) == [3]


def test_restatement_one_candidate_per_vehicle():
    r = _recs([3.0, np.nan, 1.0, 2.0], status=[0, 0, 2, 0])
    w, wr = FR.select(r, 4, 1)
    assert list(w) == [0, -1, -1, 0]
    assert wr[0].tobytes() == r[0].tobytes() and wr[3].tobytes() == r[3].tobytes() and wr[1].tobytes() == bytes(104) == wr[2].tobytes()
    w, u, st = FR.apply(r, 4, 1, np.ones((4, 4)))
    assert list(st) == [0, FR.STATUS_NAN, 2, 0]
    assert list(u[1]) == [1.0] * 4 and list(u[2]) == [1.0] * 4 and list(u[3]) == list(r["u0"][3])


def test_no_cpu_fallback():
    import torch
    import bluerov2_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(bluerov2_amd.NoDeviceError):
        bluerov2_amd.Fleet(bluerov2_amd.BatchSolver(6, bluerov2_amd.SolverOptions(20)), 3)


def test_fleet_kernels_use_no_scratch_and_the_makefile_gates_them():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "fleet_kernel.hip"], capture_output=True,
                         text=True, timeout=600).stdout
    rep = {}
    for ln in out.splitlines():
        m = re.match(r"Name: (\S+)", ln)
        if m:
            rep[m.group(1)] = {k: int(v) for k, v in re.findall(r"\|([A-Za-z ]+): (\d+)", ln)}
    kernels = ("fleet_select_kernel", "fleet_plant_kernel", "fleet_bcast_kernel")
    names = {short: r for mangled, r in rep.items() for short in kernels if re.search(r"\d+%sE" % short, mangled)}
    assert set(names) == set(kernels), sorted(rep)
    for short, r in names.items():
        assert r["scratch"] == 0 and r["lds"] == 0, (short, r)
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    srcs = mk.split("SRCS")[1].splitlines()[0]
    assert "fleet_kernel.hip" in srcs and "fleet_api.hip" in srcs
    rule = mk[mk.index("$(OUTDIR)/obj/fleet_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "fleet_plant_kernel" in rule and "rm -f $@" in rule
