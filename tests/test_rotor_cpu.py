"""The plant's rotor stage (brov_rotor_*) without a GPU: the C ABI's symbols and declarations, brov_rotor_coeffs against a 60-digit
evaluation, tests/rotor_restatement.py held to the mathematics it restates, the new kernels' resource report and the Makefile."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from rotor_restatement import RotorRestatement, pinv_allocation
from thruster_restatement import ROTOR, allocation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SYMBOLS = ["brov_rotor_coeffs", "brov_rotor_set_host", "brov_rotor_off", "brov_rotor_enabled", "brov_rotor_reset", "brov_rotor_set_state_host",
           "brov_rotor_get_state_host", "brov_rotor_last_host", "brov_rotor_get_stats_host", "brov_rotor_get_coeffs_host", "brov_rotor_eval_host",
           "brov_rotor_last_seconds"]
KERNELS = {"rotor_shift_kernel": r"\d+rotor_shift_kernelE", "rotor_eval_kernel": r"\d+rotor_eval_kernelE"}
U = 2.0 ** -52
H, TAU, NSTEPS = 0.05, 0.2, 40


def _lib():
    import bluerov2_amd
    from bluerov2_amd.solver import _load
    bluerov2_amd.build_library()
    return _load()


def _coeffs(tau, h):
    import bluerov2_amd
    bluerov2_amd.build_library()
    return bluerov2_amd.rotor_coeffs(tau, h)


# ---- symbols ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_exactly_the_twelve_names():
    import bluerov2_amd
    bluerov2_amd.build_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(brov_rotor_[a-z0-9_]+)\s*\(", txt))
    assert len(SYMBOLS) == 12 and declared == set(SYMBOLS), sorted(declared ^ set(SYMBOLS))
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("brov_rotor_"))
    assert exported == set(SYMBOLS), sorted(exported ^ set(SYMBOLS))
    assert re.search(r"int\s+brov_rotor_coeffs\(double tau, double h, double\* alpha, double\* beta\);", txt)
    assert re.search(r"int\s+brov_rotor_set_host\(brov_solver\* s, const double\* tau\s*, double h\s*,\s*const double\* cmd_lo\s*, "
                     r"const double\* cmd_hi\s*,\s*int32_t observer_applied\);", txt)
    assert re.search(r"int\s+brov_rotor_eval_host\(brov_solver\* s, const double\* commanded, const double\* state, double\* applied, "
                     r"double\* state_out\);", txt)
    assert re.search(r"int\s+brov_rotor_get_stats_host\(brov_solver\* s, double\* lag_sq\s*, int64_t\* steps\);", txt)
    assert re.search(r"int\s+brov_rotor_get_coeffs_host\(brov_solver\* s, double\* alpha\s*, double\* beta\s*, double\* h\);", txt)


def test_null_handles_are_argument_errors_with_the_calls_own_name():
    L = _lib()
    buf = (ctypes.c_double * 12)()
    p = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))
    steps = ctypes.c_int64(0)
    calls = [("brov_rotor_set_host", (None, None, 0.0, None, None, 0)), ("brov_rotor_off", (None,)), ("brov_rotor_reset", (None,)),
             ("brov_rotor_set_state_host", (None, p)), ("brov_rotor_get_state_host", (None, p)), ("brov_rotor_last_host", (None, p, p)),
             ("brov_rotor_get_stats_host", (None, p, ctypes.byref(steps))), ("brov_rotor_get_coeffs_host", (None, p, p, p)),
             ("brov_rotor_eval_host", (None, p, p, p, p)), ("brov_rotor_last_seconds", (None, p))]
    assert sorted(n for n, _ in calls) == sorted(set(SYMBOLS) - {"brov_rotor_coeffs", "brov_rotor_enabled"})   # every entry point with a handle
    for name, args in calls:
        assert getattr(L, name)(*args) == ERR_ARG, (name, args)
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())   # the text of THIS call
    assert L.brov_rotor_enabled(None) == 0


def test_python_names_exist():
    import bluerov2_amd
    for name in ("set_rotors", "rotor_off", "rotor_enabled", "rotor_reset", "rotor_state", "set_rotor_state", "rotor_last", "rotor_stats",
                 "rotor_coeffs", "rotor_eval", "rotor_last_seconds"):
        assert callable(getattr(bluerov2_amd.BatchSolver, name)), name
    assert callable(bluerov2_amd.rotor_coeffs) and "rotor_coeffs" in bluerov2_amd.__all__


# ---- coefficients ------------------------------------------------------------------------------------------------------------------------------
def test_coefficients_against_a_sixty_digit_evaluation():
    """alpha: relative error <= (1 + h / tau) 2^-52 where alpha > 1e-300 (one rounding of the quotient carried through exp, plus libm's own
    ulp); beta: <= 2 * 2^-52 (the quotient, expm1 and the division).  20 000 draws, h in [1e-4, 1], tau in [1e-4, 100], log-uniform."""
    import mpmath as mp
    mp.mp.dps = 60
    L = _lib()
    rng = np.random.default_rng(2026)
    n = 20000
    hs = np.exp(rng.uniform(math.log(1e-4), math.log(1.0), n))
    taus = np.exp(rng.uniform(math.log(1e-4), math.log(100.0), n))
    al, be = ctypes.c_double(0.0), ctypes.c_double(0.0)
    worst_a = worst_b = 0.0
    checked_a = 0
    for h, tau in zip(hs.tolist(), taus.tolist()):
        assert L.brov_rotor_coeffs(tau, h, ctypes.byref(al), ctypes.byref(be)) == 0
        x = mp.mpf(h) / mp.mpf(tau)
        a_ref = mp.exp(-x)
        b_ref = (1 - a_ref) / x
        if al.value > 1e-300:
            ea = float(abs(mp.mpf(al.value) - a_ref) / a_ref) / ((1.0 + h / tau) * U)
            worst_a = max(worst_a, ea)
            checked_a += 1
        eb = float(abs(mp.mpf(be.value) - b_ref) / b_ref) / (2.0 * U)
        worst_b = max(worst_b, eb)
    print(f"alpha: worst {worst_a:.3f} of (1 + h/tau) 2^-52 over {checked_a} draws; beta: worst {2.0 * worst_b:.3f} of 2^-52 (allowed 2)")
    assert checked_a > n // 2
    assert worst_a <= 1.0 and worst_b <= 1.0


def test_tau_zero_and_the_refusals_of_the_coefficients():
    L = _lib()
    al, be = ctypes.c_double(7.0), ctypes.c_double(7.0)
    assert L.brov_rotor_coeffs(0.0, 0.05, ctypes.byref(al), ctypes.byref(be)) == 0
    assert al.value == 0.0 and be.value == 0.0 and math.copysign(1.0, al.value) == 1.0 and math.copysign(1.0, be.value) == 1.0
    assert _coeffs(0.0, 1.0) == (0.0, 0.0)
    for tau, h in ((-0.1, 0.05), (math.nan, 0.05), (math.inf, 0.05), (-math.inf, 0.05), (0.2, 0.0), (0.2, -0.05), (0.2, math.nan), (0.2, math.inf),
                   (0.0, 0.0), (0.0, math.nan)):
        al.value = be.value = 7.0
        assert L.brov_rotor_coeffs(tau, h, ctypes.byref(al), ctypes.byref(be)) == ERR_ARG, (tau, h)
        assert al.value == 7.0 and be.value == 7.0
        with pytest.raises(ValueError):
            _coeffs(tau, h)
    a, b = _coeffs(0.2, 0.05)
    assert 0.0 < a < 1.0 and a < b < 1.0                      # the mean lies between the end value and the command
    a, b = _coeffs(1e-6, 0.05)
    assert a == 0.0 and 0.0 < b < 1e-4                        # alpha underflows to 0, beta = 1 / x stays: no copy


# ---- the restatement, held to mathematics ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def constant_run():
    """constant commands from r = 0 over 40 steps with the library's coefficients for tau = 0.2, h = 0.05: (c [6], r_n [6], m [40][6], alpha)"""
    a, b = _coeffs(TAU, H)
    c = np.array([[35.0, -12.5, 1540.0, -0.001, 3.3e-7, 97.0 / 3.0]])
    rs = RotorRestatement(1, a, b)
    ms = []
    for _ in range(NSTEPS):
        _, m = rs.step(np.zeros((1, 4)), c)
        ms.append(m[0])
    assert rs.steps == NSTEPS
    return c[0], rs.r[0].copy(), np.array(ms), a


def test_constant_command_end_state_and_impulse(constant_run):
    """r_n within 4 n 2^-53 |c| of c (1 - alpha^n) (three roundings per step and some margin); h sum_k m_k within the same bound of the exact
    impulse c (n h - tau (1 - alpha^n)).  alpha = exp(-h / tau) at 60 digits from the doubles h and tau."""
    import mpmath as mp
    mp.mp.dps = 60
    c, rn, ms, _ = constant_run
    an = mp.exp(-mp.mpf(H) / mp.mpf(TAU)) ** NSTEPS
    for i in range(6):
        bound = 4 * NSTEPS * 2.0 ** -53 * abs(c[i])
        r_ref = mp.mpf(c[i]) * (1 - an)
        imp_ref = mp.mpf(c[i]) * (NSTEPS * mp.mpf(H) - mp.mpf(TAU) * (1 - an))
        imp = mp.mpf(H) * sum(mp.mpf(float(v)) for v in ms[:, i])
        er, ei = float(abs(mp.mpf(rn[i]) - r_ref)), float(abs(imp - imp_ref))
        print(f"c = {c[i]:.6g}: |r_n - ref| = {er / bound:.3f}, |impulse - ref| = {ei / bound:.3f} of the bound {bound:.3e}")
        assert er <= bound and ei <= bound, (i, er, ei, bound)
    assert np.all(np.abs(rn) < np.abs(c)) and np.all(np.sign(rn) == np.sign(c))


def test_non_finite_commands_move_nothing():
    a, b = _coeffs(TAU, H)
    rs = RotorRestatement(3, a, b)
    rs.step(np.zeros((3, 4)), np.full((3, 6), 10.0))
    r0, lag0 = rs.r.copy(), rs.lag_sq.copy()
    t = np.array([[np.nan] * 6, [np.inf] * 6, [-np.inf, np.nan, np.inf, -np.inf, np.nan, np.inf]])
    u0, m = rs.step(np.ones((3, 4)), t)
    assert np.array_equal(rs.r, r0) and np.array_equal(m, r0) and np.array_equal(rs.lag_sq, lag0)   # m = r' = r, (c - m) = 0
    assert np.isfinite(u0).all() and np.array_equal(u0, pinv_allocation(r0))
    # ... also under tau = 0, where the command would be copied: the state holds, nothing non-finite is stored
    rz = RotorRestatement(1, 0.0, 0.0)
    rz.step(np.zeros((1, 4)), np.full((1, 6), 4.0))
    _, m = rz.step(np.zeros((1, 4)), np.full((1, 6), np.nan))
    assert np.array_equal(m, np.full((1, 6), 4.0)) and np.array_equal(rz.r, m)
    # a limit turns an infinite command into a finite one, which does move the rotor
    rl = RotorRestatement(1, a, b, lo=-50.0, hi=50.0)
    _, m = rl.step(np.zeros((1, 4)), np.full((1, 6), np.inf))
    assert np.array_equal(m, 50.0 + b * (0.0 - 50.0) * np.ones((1, 6)))


def test_minus_zero_survives_tau_zero_and_the_record_is_kept():
    rz = RotorRestatement(2, 0.0, 0.0)
    t = np.array([[-0.0, 0.0, -0.0, 5.0, -7.0, -0.0], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    u_in = np.array([[0.123, -0.0, 0.3, 1e-300], [9.0, 8.0, 7.0, 6.0]])
    u0, m = rz.step(u_in, t)
    assert m.tobytes() == t.tobytes() and rz.r.tobytes() == t.tobytes()     # (array_equal would take -0 for +0)
    assert u0.tobytes() == u_in.tobytes()                                   # the whole record copied: u0 is not recomputed
    assert not rz.lag_sq.any()
    # with a time constant, c + beta * d turns -0 into +0 (which is why tau = 0 copies)
    a, b = _coeffs(TAU, H)
    rs = RotorRestatement(1, a, b)
    _, m = rs.step(np.zeros((1, 4)), np.full((1, 6), -0.0))
    assert not np.signbit(m).any()
    # one rotor with a time constant: the record is no copy any more, u0 is the left inverse of m
    al, be = np.zeros((1, 6)), np.zeros((1, 6)); al[0, 2], be[0, 2] = a, b
    rm = RotorRestatement(1, al, be)
    u0, m = rm.step(u_in[1:], t[1:])
    assert np.array_equal(m[0, [0, 1, 3, 4, 5]], t[1, [0, 1, 3, 4, 5]]) and m[0, 2] == 3.0 + b * (0.0 - 3.0)
    assert np.array_equal(u0, pinv_allocation(m)) and not np.array_equal(u0, u_in[1:])


def test_clamp_acts_ahead_of_the_lag():
    a, b = _coeffs(TAU, H)
    lo, hi = np.array([-10.0, -10, -10, -5, -5, -5]), np.array([10.0, 10, 10, 5, 5, 5])
    rs, free = RotorRestatement(1, a, b, lo, hi), RotorRestatement(1, a, b)
    t = np.array([[100.0, -100.0, 3.0, 7.0, -7.0, 0.5]])
    cl = np.array([[10.0, -10.0, 3.0, 5.0, -5.0, 0.5]])
    for _ in range(30):
        _, m = rs.step(np.zeros((1, 4)), t)
        _, mf = free.step(np.zeros((1, 4)), cl)
        assert np.array_equal(m, mf)                           # the stage with limits on t is the stage without on clamp(t)
    assert np.all(np.abs(rs.r) <= np.abs(cl)) and np.abs(rs.r - cl).max() < 0.01 * np.abs(cl).max()
    # lag_sq counts c - m, the clamped command against the applied thrust, not the raw command
    assert rs.lag_sq[0] == free.lag_sq[0] and rs.lag_sq[0] < 30 * 6 * 10.0 ** 2
    # tau = 0 with limits: the clamped command at once, and u0 follows the clamped thrusts
    rz = RotorRestatement(1, 0.0, 0.0, lo, hi)
    u0, m = rz.step(np.full((1, 4), 0.5), t)
    assert np.array_equal(m, cl) and np.array_equal(u0, pinv_allocation(cl))


def test_left_inverse_of_the_allocation():
    """pinv(alloc(u)) == u to 2 ulp for random u.  The four horizontal thrusts are rounded at the magnitude S / rc, S = |u0| + |u1| + |u3|
    (one of the four sign patterns of the allocation attains it), so the unit is 2^-52 S for the three horizontal inputs and 2^-52 |u2| for
    the vertical one, the units of the coefficient bounds above."""
    rng = np.random.default_rng(7)
    worst = np.zeros(4)
    for u in (rng.uniform(-1.0, 1.0, (100000, 4)), rng.normal(size=(100000, 4)) * 30.0,
              rng.normal(size=(100000, 4)) * np.exp(rng.normal(size=(100000, 4)) * 3.0)):
        v = pinv_allocation(allocation(u))
        S = np.abs(u[:, 0]) + np.abs(u[:, 1]) + np.abs(u[:, 3])
        unit = np.stack([S, S, np.abs(u[:, 2]), S], axis=1) * U
        worst = np.maximum(worst, (np.abs(v - u) / unit).max(axis=0))
    print("worst |pinv(alloc(u)) - u| in units of 2^-52 S:", worst)
    assert np.all(worst <= 2.0)
    assert ROTOR == 0.026546960744430276


# ---- resources -----------------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch_no_lds_and_are_built():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "rotor_kernel.hip"], capture_output=True,
                         text=True, timeout=600).stdout
    rep = {}
    for ln in out.splitlines():
        m = re.match(r"Name: (\S+)", ln)
        if m:
            assert m.group(1) not in rep
            rep[m.group(1)] = {k: int(v) for k, v in re.findall(r"\|([A-Za-z ]+): (\d+)", ln)}
    for short, pat in KERNELS.items():
        hit = [r for m, r in rep.items() if re.search(pat, m)]
        assert len(hit) == 1, (short, sorted(rep))
        print(short, hit[0])
        assert hit[0]["scratch"] == 0 and hit[0]["lds"] == 0, (short, hit[0])
    assert len(rep) == 2, sorted(rep)
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "rotor_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/rotor_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    assert "rotor_shift_kernel" in rule and "rotor_eval_kernel" in rule
