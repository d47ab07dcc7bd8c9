"""The inter-vehicle clearance term of the fleet loop (brov_clearance_*) without a GPU: the C ABI's symbols, the argument checks that need
no device, hand-computed answers of the numpy restatement the kernels are held to, and the kernels' resource report."""
import ctypes
import os
import re
import subprocess

import numpy as np

import clearance_restatement as CR
import fleet_restatement as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SYMBOLS = ["brov_clearance_set", "brov_clearance_off", "brov_clearance_enabled", "brov_clearance_set_plan_host", "brov_clearance_get_plan_host",
           "brov_clearance_eval_device", "brov_clearance_eval_host", "brov_clearance_get_stats_host", "brov_clearance_last_seconds",
           "brov_clearance_dev_set_slices", "brov_clearance_dev_slices"]
INF, NAN = np.inf, np.nan


def test_library_exports_and_header_declares_exactly_the_clearance_family():
    import bluerov2_amd
    bluerov2_amd.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split())
    assert not [n for n in SYMBOLS if n not in exported]
    assert sorted(n for n in exported if n.startswith("brov_clearance_")) == sorted(SYMBOLS)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(brov_clearance_[a-z0-9_]+)\s*\(", txt))) == sorted(SYMBOLS)
    assert re.search(r"int\s+brov_clearance_set\(brov_fleet\* f, double radius, double weight, int shift\);", txt)
    assert re.search(r"int\s+brov_clearance_eval_device\(brov_fleet\* f, const double\* x, const brov_result\* rec, double\* d2min, "
                     r"brov_result\* out, void\* stream\);", txt)


def test_null_arguments_are_argument_errors_named_after_the_call():
    import bluerov2_amd
    from bluerov2_amd.fleet import _fleet_lib
    bluerov2_amd.build_library()
    L = _fleet_lib()
    d = (ctypes.c_double * 4)()
    calls = {
        "brov_clearance_set": lambda: L.brov_clearance_set(None, 1.0, 1.0, 1),
        "brov_clearance_off": lambda: L.brov_clearance_off(None),
        "brov_clearance_set_plan_host": lambda: L.brov_clearance_set_plan_host(None, d),
        "brov_clearance_get_plan_host": lambda: L.brov_clearance_get_plan_host(None, d),
        "brov_clearance_eval_device": lambda: L.brov_clearance_eval_device(None, None, None, None, None, None),
        "brov_clearance_eval_host": lambda: L.brov_clearance_eval_host(None, None, d, None),
        "brov_clearance_get_stats_host": lambda: L.brov_clearance_get_stats_host(None, None, None, None),
        "brov_clearance_last_seconds": lambda: L.brov_clearance_last_seconds(None, d),
        "brov_clearance_dev_set_slices": lambda: L.brov_clearance_dev_set_slices(None, 1),
    }
    for name, call in calls.items():
        assert call() == ERR_ARG, name
        assert L.brov_fleet_last_error().decode().startswith(name + ":"), (name, L.brov_fleet_last_error())
    assert L.brov_clearance_enabled(None) == 0 and L.brov_clearance_dev_slices(None) == 0
    for name in ("set_clearance", "clearance_off", "clearance_enabled", "set_plan", "plan", "clearance_eval", "clearance_stats",
                 "clearance_seconds", "clearance_slices"):
        assert callable(getattr(bluerov2_amd.Fleet, name))


def _paths(points):
    """x [B, N + 1, 12] whose positions are `points` [B, N + 1, 3]; the other columns hold numbers nobody may read"""
    points = np.asarray(points, dtype=np.float64)
    x = np.full(points.shape[:2] + (12,), 1e30)
    x[..., :3] = points
    return x


def _recs(cost, status=None):
    cost = np.asarray(cost, dtype=np.float64)
    r = np.zeros(cost.size, dtype=FR.RESULT_DTYPE)
    r["cost"] = cost
    r["status"] = 0 if status is None else status
    r["u0"] = np.arange(cost.size * 4).reshape(-1, 4) + 1.0
    r["kkt"] = np.arange(cost.size) * 0.5
    r["qp_iter"] = 3
    r["thrust"] = 0.25
    return r


def test_two_vehicles_at_a_known_separation():
    # V = 2, C = 1, N = 1: vehicle 0 moves (0,0,0) -> (5,0,0), vehicle 1 (4,4,2) -> (1,3,4)
    x = _paths([[[0, 0, 0], [5, 0, 0]], [[4, 4, 2], [1, 3, 4]]])
    plan = x[:, :, :3].copy()
    d = CR.d2min(x, plan, 2, 1, shift=0)
    assert list(d) == [36.0, 36.0]                       # stage 0: 16 + 16 + 4 = 36; stage 1: 16 + 9 + 16 = 41
    # shift = 1: every stage is held against the peer's LAST stage (k + 1 clamps at N = 1)
    d = CR.d2min(x, plan, 2, 1, shift=1)
    assert list(d) == [26.0, 21.0]                       # against (1,3,4): 26 and 41; against (5,0,0): 1 + 16 + 4 = 21 and 41
    assert np.array_equal(CR.d2min_fast(x, plan, 2, 1, 1), d) and np.array_equal(CR.d2min_fast(x, plan, 2, 1, 0), CR.d2min(x, plan, 2, 1, 0))


def test_shift_one_reads_the_peer_one_stage_ahead_and_clamps_at_the_last_stage():
    # N = 2: the peer's plan is (10,0,0), (20,0,0), (30,0,0); the candidate sits at (0,0,0), (19,0,0), (26,0,0)
    x = _paths([[[0, 0, 0], [19, 0, 0], [26, 0, 0]], [[10, 0, 0], [20, 0, 0], [30, 0, 0]]])
    plan = x[:, :, :3].copy()
    assert CR.d2min(x, plan, 2, 1, 0)[0] == 1.0          # stage 1 against stage 1
    assert CR.d2min(x, plan, 2, 1, 1)[0] == 16.0         # stages against 1, 2, 2: 400, 121, 16
    assert CR.d2min(x, plan, 2, 1, 2)[0] == 16.0         # stages against 2, 2, 2: 900, 121, 16


def test_a_candidate_on_its_own_vehicles_plan_does_not_score_zero():
    # V = 2, C = 2: candidate 0 of vehicle 0 IS vehicle 0's plan; the peer is 3 away
    own = [[0, 0, 0], [1, 0, 0]]
    x = _paths([own, [[0, 1, 0], [1, 1, 0]], [[0, 0, 3], [1, 0, 3]], [[0, 0, 3], [1, 0, 3]]])
    plan = np.array([own, [[0, 0, 3], [1, 0, 3]]], dtype=np.float64)
    d = CR.d2min(x, plan, 2, 2, 0)
    assert list(d) == [9.0, 10.0, 9.0, 9.0]              # candidates 2 and 3 lie on THEIR vehicle's plan too and see only vehicle 0
    assert np.array_equal(CR.d2min_fast(x, plan, 2, 2, 0), d)


def test_a_nan_peer_is_skipped_and_one_vehicle_gives_inf():
    x = _paths([[[0, 0, 0]] * 2, [[NAN, 0, 0]] * 2, [[0, 5, 0]] * 2])
    plan = x[:, :, :3].copy()
    d = CR.d2min(x, plan, 3, 1, 0)
    assert d[0] == 25.0 and d[2] == 25.0                 # vehicle 1's plan is not a number: skipped
    assert d[1] == INF                                   # its own path is NaN: every distance is, nothing is below +Inf
    assert np.array_equal(CR.d2min_fast(x, plan, 3, 1, 0), d)
    one = CR.d2min(x[:2], plan[:1], 1, 2, 1)
    assert list(one) == [INF, INF] and list(CR.d2min_fast(x[:2], plan[:1], 1, 2, 1)) == [INF, INF]


def test_penalty_with_a_finite_weight():
    r = _recs([10.0, 10.0, 10.0, -3.0])
    d2 = np.array([1.0, 4.0, 3.75, 0.0])
    out = CR.rescore(r, d2, radius=2.0, weight=8.0)      # r2 = 4
    assert list(out["cost"]) == [10.0 + 8.0 * 3.0, 10.0, 10.0 + 8.0 * 0.25, -3.0 + 32.0]     # d2min == r2 pays nothing
    for name in ("u0", "kkt", "status", "qp_iter", "thrust"):
        assert out[name].tobytes() == r[name].tobytes()
    assert r["cost"][0] == 10.0                          # the input is left alone
    # the three operations are rounded separately: r2 - d2 = 0.25 - 0.01 first, then the product, then the sum
    r = _recs([0.1])
    out = CR.rescore(r, np.array([0.01]), radius=0.5, weight=0.3)
    assert out["cost"][0] == np.float64(0.1) + np.float64(0.3) * (np.float64(0.25) - np.float64(0.01))


def test_an_infinite_weight_prices_a_group_out_and_the_select_returns_minus_one():
    # V = 2, C = 2: both candidates of vehicle 0 are inside the radius, one of vehicle 1 is
    r = _recs([1.0, 2.0, 3.0, 4.0])
    d2 = np.array([0.5, 0.0, 0.9, 1.0])
    out = CR.rescore(r, d2, radius=1.0, weight=INF)
    assert list(out["cost"]) == [INF, INF, INF, 4.0]
    w, _ = FR.select(out, 2, 2)
    assert list(w) == [-1, 1]
    w, u, st = FR.apply(out, 2, 2, np.full((2, 4), 0.5))
    assert list(st) == [FR.STATUS_NAN, 0] and list(u[0]) == [0.5] * 4          # priced out: held, as when all had failed
    assert list(FR.select(r, 2, 2)[0]) == [0, 0]                                # ... and without the term both had a winner


def test_nan_and_infinite_costs():
    r = _recs([NAN, NAN, -INF, -INF, INF])
    d2 = np.array([0.0, 9.0, 0.0, 0.0, 0.0])
    fin = CR.rescore(r, d2, radius=1.0, weight=2.0)
    assert np.isnan(fin["cost"][0]) and np.isnan(fin["cost"][1])                # a NaN cost stays NaN, penalised or not
    assert fin["cost"][2] == -INF and fin["cost"][4] == INF
    hard = CR.rescore(r, d2, radius=1.0, weight=INF)
    assert np.isnan(hard["cost"][0]) and hard["cost"][4] == INF
    # -Inf + Inf is not a number; it is written as the quiet NaN whatever the processor makes of it
    assert hard["cost"][2:4].view(np.uint64).tolist() == [0x7ff8000000000000] * 2
    assert fin["cost"][1:2].tobytes() == r["cost"][1:2].tobytes()               # outside the radius: the bytes are copied
    # a cost that is NaN already keeps its bytes inside the radius too, sign and payload included
    odd = np.array([0xfff8000000000123, 0x7ff800000000beef], dtype=np.uint64).view(np.float64)
    r = _recs(odd)
    for weight in (2.0, INF):
        out = CR.rescore(r, np.zeros(2), radius=1.0, weight=weight)
        assert out.tobytes() == r.tobytes()


def test_publish_and_statistics():
    V, C, N = 3, 2, 2
    rng = np.random.default_rng(3)
    x = rng.normal(size=(V * C, N + 1, 12))
    plan = rng.normal(size=(V, N + 1, 3))
    winner = np.array([1, -1, 0], dtype=np.int32)
    new = CR.publish(plan, x, winner, V, C, shift=1)
    assert np.array_equal(new[0], x[1, :, :3]) and np.array_equal(new[2], x[4, :, :3])
    assert np.array_equal(new[1], plan[1][[1, 2, 2]])                           # advanced by one stage, the last one repeated
    assert np.array_equal(CR.publish(plan, x, winner, V, C, shift=0)[1], plan[1])
    assert np.array_equal(CR.publish(plan, x, winner, V, C, shift=2)[1], plan[1][[2, 2, 2]])
    d2 = np.array([9.0, 0.5, 1.0, 1.0, 4.0, 0.0])
    st = CR.stats(CR.fresh_stats(V), d2, winner, V, C, radius=1.5)
    assert list(st["last_d2"]) == [0.5, -1.0, 4.0] and list(st["min_d2"]) == [0.5, INF, 4.0] and list(st["below"]) == [1, 0, 0]
    st = CR.stats(st, d2, np.array([0, 0, -1], dtype=np.int32), V, C, radius=1.5)
    assert list(st["last_d2"]) == [9.0, 1.0, -1.0] and list(st["min_d2"]) == [0.5, 1.0, 4.0] and list(st["below"]) == [1, 1, 0]


def test_clearance_kernels_use_no_scratch_and_the_makefile_gates_them():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "clearance_kernel.hip"], capture_output=True,
                         text=True, timeout=600).stdout
    rep = {}
    for ln in out.splitlines():
        m = re.match(r"Name: (\S+)", ln)
        if m:
            rep[m.group(1)] = {k: int(v) for k, v in re.findall(r"\|([A-Za-z ]+): (\d+)", ln)}
    kernels = ("clearance_dist_kernel", "clearance_rescore_kernel", "clearance_publish_kernel")
    names = {short: r for mangled, r in rep.items() for short in kernels if re.search(r"\d+%sE" % short, mangled)}
    assert set(names) == set(kernels), sorted(rep)
    for short, r in names.items():
        assert r["scratch"] == 0 and r["VGPRs Spill"] == 0, (short, r)
    assert names["clearance_dist_kernel"]["lds"] == 4 * 64 * 8                  # the four wavefronts' minima, nothing else
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "clearance_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/clearance_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    for k in kernels:
        assert k in rule
