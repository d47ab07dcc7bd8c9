"""The plant's ocean current (brov_current_*) without a GPU: the C ABI's symbols and declarations, the argument checks that need no device,
the BatchSolver methods, the new kernels' resource report and the Makefile's gate, and the numpy restatement of tests/current_restatement.py
against what the model says about it: still water is the plant under a wrench, a vehicle adrift takes the water's velocity, the
Gauss-Markov state without noise relaxes geometrically, and the case chosen for the GPU test meets both of its bounds."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np

import current_restatement as CR
from current_restatement import CurrentRestatement
from wrench_restatement import rk4_under_wrench, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SYMBOLS = ["brov_current_constant_host", "brov_current_table_host", "brov_current_gauss_markov_host", "brov_current_off", "brov_current_mode",
           "brov_current_eval_host", "brov_current_get_state_host", "brov_current_set_state_host", "brov_current_last_host",
           "brov_current_last_seconds"]
KERNELS = {"current_eval_kernel": r"\d+current_eval_kernelE", "plant_current_kernel<0, 0>": r"\d+plant_current_kernelILb0ELb0EE",
           "plant_current_kernel<0, 1>": r"\d+plant_current_kernelILb0ELb1EE", "plant_current_kernel<1, 0>": r"\d+plant_current_kernelILb1ELb0EE",
           "plant_current_kernel<1, 1>": r"\d+plant_current_kernelILb1ELb1EE"}
P_NOMINAL = np.array([0, 0, 0, 0, 1.7182, 0, 5.468, 0.4006, -11.7391, -20, -31.8678, -5, -18.18, -21.66, -36.99, -1.55])


def _lib():
    import bluerov2_amd
    from bluerov2_amd.solver import _load
    bluerov2_amd.build_library()
    return _load()


def test_header_declares_and_library_exports_exactly_the_ten_names():
    import bluerov2_amd
    bluerov2_amd.build_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(brov_current_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(SYMBOLS), sorted(declared ^ set(SYMBOLS))
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("brov_current_"))
    assert exported == set(SYMBOLS), sorted(exported ^ set(SYMBOLS))
    assert re.search(r"int\s+brov_current_table_host\(brov_solver\* s, const double\* tab\s*, int rows, const double\* gain\s*\);", txt)
    assert re.search(r"int\s+brov_current_gauss_markov_host\(brov_solver\* s, uint64_t seed, const double\* mean\s*, const double\* mu\s*, "
                     r"const double\* amp\s*,\s*const double\* lo\s*, const double\* hi\s*, double step\s*\);", txt)
    assert re.search(r"int\s+brov_current_eval_host\(brov_solver\* s, int64_t tick, double\* v\s*\);", txt)
    modes = dict(re.findall(r"#define (BROV_CURRENT_[A-Z_]+) (\d+)", txt))
    assert modes == {"BROV_CURRENT_OFF": "0", "BROV_CURRENT_CONSTANT": "1", "BROV_CURRENT_TABLE": "2", "BROV_CURRENT_GAUSS_MARKOV": "3"}
    assert (bluerov2_amd.CURRENT_OFF, bluerov2_amd.CURRENT_CONSTANT, bluerov2_amd.CURRENT_TABLE, bluerov2_amd.CURRENT_GAUSS_MARKOV) == (0, 1, 2, 3)
    assert (CR.OFF, CR.CONSTANT, CR.TABLE, CR.GAUSS_MARKOV) == (0, 1, 2, 3)


def test_null_handles_are_argument_errors_with_the_calls_own_name():
    L = _lib()
    three = (ctypes.c_double * 3)()
    p3 = ctypes.cast(three, ctypes.POINTER(ctypes.c_double))
    sec = ctypes.c_double(0.0)
    calls = [("brov_current_constant_host", (None, p3)), ("brov_current_table_host", (None, p3, 1, None)),
             ("brov_current_gauss_markov_host", (None, 0, p3, p3, p3, None, None, 0.05)), ("brov_current_off", (None,)),
             ("brov_current_eval_host", (None, 0, p3)), ("brov_current_get_state_host", (None, p3)), ("brov_current_set_state_host", (None, p3)),
             ("brov_current_last_host", (None, p3)), ("brov_current_last_seconds", (None, ctypes.byref(sec)))]
    for name, args in calls:
        assert getattr(L, name)(*args) == ERR_ARG, (name, args)
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())   # the text of THIS call
    assert L.brov_current_mode(None) == 0


def test_batch_solver_methods_and_the_angle_convention():
    import bluerov2_amd
    for name in ("set_current", "current_off", "current_mode", "current", "current_state", "set_current_state", "current_last",
                 "current_last_seconds"):
        assert callable(getattr(bluerov2_amd.BatchSolver, name)), name
    # the plugin's convention, at angles whose sines and cosines are plain: h = 90 deg turns the current into +y, v = 90 deg into +z
    v = bluerov2_amd.current_from_angles(2.0, 0.0, 0.0)
    assert np.array_equal(v, [2.0, 0.0, 0.0])
    assert np.allclose(bluerov2_amd.current_from_angles(2.0, math.pi / 2, 0.0), [0.0, 2.0, 0.0], atol=1e-15)
    assert np.allclose(bluerov2_amd.current_from_angles(2.0, 0.3, math.pi / 2), [0.0, 0.0, 2.0], atol=1e-15)
    h, e = 0.7, -0.2
    want = [0.4 * math.cos(h) * math.cos(e), 0.4 * math.sin(h) * math.cos(e), 0.4 * math.sin(e)]
    assert np.allclose(bluerov2_amd.current_from_angles(0.4, h, e), want, rtol=1e-15) and np.allclose(CR.current_from_angles(0.4, h, e), want, rtol=1e-15)
    assert bluerov2_amd.current_from_angles([0.1, 0.2], 0.0, 0.0).shape == (2, 3)


def test_new_kernels_use_no_scratch_and_the_makefile_gates_them():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "plant_current.hip"], capture_output=True,
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
    assert "plant_current.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/plant_current.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    assert "plant_current_kernel" in rule and "current_eval_kernel" in rule


def test_still_water_is_the_plant_under_a_wrench(oracle):
    rng = np.random.default_rng(4)
    for substeps in (1, 4):
        x = rng.normal(size=12) * 0.2
        u, w = rng.uniform(-5, 5, 4), rng.uniform(-20, 20, 6)
        p = P_NOMINAL.copy(); p[:4] = rng.uniform(-10, 10, 4)
        a = CR.rk4_under_current(oracle, x, u, p, w, np.zeros(3), 0.05, substeps)
        assert np.array_equal(a, rk4_under_wrench(oracle, x, u, p, w, 0.05, substeps))
        # ... and moving water is not: rows 6..8 alone differ at the first stage
        f0, f1 = CR.f_under_current(oracle, x, u, p, w, np.zeros(3)), CR.f_under_current(oracle, x, u, p, w, np.array([0.3, -0.2, 0.1]))
        assert np.array_equal(np.delete(f0, [6, 7, 8]), np.delete(f1, [6, 7, 8])) and np.abs(f0[6:9] - f1[6:9]).min() > 1e-3


def test_a_vehicle_adrift_takes_the_waters_velocity(oracle):
    """u = 0, level attitude, a constant horizontal current of 0.4 m/s: nothing but drag acts in the horizontal plane, so the velocity through
    the water decays, and the decay is at least that of the linear damping alone (the quadratic term only adds to it), whose slowest axis is
    surge: d/dt ur = -(11.7391 / (11.26 + 1.7182)) ur.  After 10 s (200 ticks of 0.05 s) that leaves at most 0.4 e^(-10 * 11.7391 / 12.9782)
    = 4.7e-5 m/s, the bound; the restatement shows 2.4e-5.  The attitude stays level (no moment acts) and the vehicle rises slowly (0.66 N)."""
    vc = CR.current_from_angles(0.4, 0.7, 0.0)
    x = np.zeros(12)
    gap = []
    for k in range(200):
        x = CR.rk4_under_current(oracle, x, np.zeros(4), P_NOMINAL, np.zeros(6), vc, 0.05)
        gap.append(np.abs((rotation(x) @ x[6:9])[:2] - vc[:2]).max())
    bound = 0.4 * math.exp(-10.0 * 11.7391 / (11.26 + 1.7182))
    print(f"|v_ground - vc| after 10 s: {gap[-1]:.2e} (bound {bound:.2e})")
    assert gap[-1] < bound < 5e-5 and gap[0] > 0.25 and all(b < a for a, b in zip(gap, gap[1:]))
    assert not x[3:6].any() and abs(x[8]) < 0.05
    # the way the vehicle went: downstream
    assert 0.8 * 10.0 * vc[0] < x[0] < 10.0 * vc[0] and 0.8 * 10.0 * vc[1] < x[1] < 10.0 * vc[1]


def test_gauss_markov_without_noise_relaxes_geometrically():
    """amp = 0: c_k = mean + (1 - step * mu)^k (c_0 - mean).  A step of the restatement rounds four times (c - mean, mu *, step *, c -), each by
    at most 2^-53 of a magnitude below |c_0| + |mean|, and the map contracts; the closed form rounds its power about k times: 8 k 2^-53
    (|c_0| + |mean|) bounds the difference with room to spare."""
    B, k_end = 5, 200
    rng = np.random.default_rng(2)
    mean, c0 = rng.uniform(-0.4, 0.4, (B, 3)), rng.uniform(-0.4, 0.4, (B, 3))
    mu, step = np.array([0.5, 2.0, 0.0]), 0.05
    r = CurrentRestatement(B).gauss_markov(seed=9, mean=mean, mu=mu, amp=0.0, step=step)
    assert np.array_equal(r.state(0), mean)                      # entering the mode: the mean
    r.set_state(c0)
    for k in range(k_end):
        assert np.array_equal(r.step(k), r.last)
        want = mean + (1.0 - step * mu) ** (k + 1) * (c0 - mean)
        assert np.abs(r.state(k + 1) - want).max() <= 8 * (k + 1) * 2.0 ** -53 * (np.abs(c0) + np.abs(mean)).max(), k
    assert np.array_equal(r.state(0)[:, 2], c0[:, 2])            # mu = 0: the axis stays where it was
    assert not r.clamped_lo.any() and not r.clamped_hi.any()     # the default bounds, -+5 m/s, are far away


def test_draws_are_uniform_counter_based_and_the_gpu_case_meets_both_bounds():
    B = 96
    r = CurrentRestatement(B).gauss_markov(mean=CR.gm_case_mean(B), **CR.GM_CASE)
    U = np.stack([r.uniform(k) for k in range(CR.GM_TICK0, CR.GM_TICK0 + CR.GM_STEPS)])
    assert U.min() >= 0.0 and U.max() < 1.0 and abs(U.mean() - 0.5) < 0.01 and abs(U.var() - 1 / 12) < 0.005
    assert np.array_equal(r.uniform(CR.GM_TICK0), U[0]) and len(np.unique(U)) == U.size      # a pure function of (seed, b, k, i)
    seen = []
    for k in range(CR.GM_TICK0, CR.GM_TICK0 + CR.GM_STEPS):
        r.step(k)
        seen.append(r.state(k + 1))
    seen = np.array(seen)
    assert (seen >= r.lo).all() and (seen <= r.hi).all()
    # the condition on the inputs of tests/test_gpu_current.py: every axis clamps on either side, some instances wander into a bound after
    # the first step, and some never meet one
    print("clamped at lo / hi per axis:", r.clamped_lo.sum(0), r.clamped_hi.sum(0))
    assert (r.clamped_lo.sum(0) >= 1).all() and (r.clamped_hi.sum(0) >= 1).all()
    per_inst = (r.clamped_lo + r.clamped_hi).sum(1)
    assert (per_inst == 0).sum() >= 1 and ((per_inst > 0) & (per_inst < 3 * CR.GM_STEPS)).sum() >= 10


def test_table_repeats_its_last_row_and_scales_by_one_rounded_product():
    B = 3
    tab = np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]])
    gain = np.array([1.0, 3.0, -0.1])
    r = CurrentRestatement(B).table(tab, gain)
    assert np.array_equal(r.current(1), tab[1][None, :] * gain[:, None]) and np.array_equal(r.current(2), r.current(10 ** 6))
    assert np.array_equal(r.current(-3), r.current(0)) and np.array_equal(CurrentRestatement(B).table(tab).current(1), np.tile(tab[1], (B, 1)))
    assert not CurrentRestatement(B).current(5).any()
