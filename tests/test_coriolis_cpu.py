"""The plant's Coriolis stage (brov_coriolis_*) without a GPU: the C ABI's symbols and declarations, the argument checks that need no device,
the BatchSolver methods, the new kernels' resource report and the Makefile's gate, and the numpy restatement of tests/coriolis_restatement.py
against what rigid-body mechanics says about it: it is rows X, Y, Z, N of -C_RB(nu) nu - C_A(nu_r) nu_r, it does no work, it is the formulas
at 60 digits to a few roundings, and on the CPU loop it removes the phantom disturbance the observer reports against the OCP-model plant."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np

import coriolis_restatement as CO
import model_exact
from current_restatement import rk4_under_current

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SYMBOLS = ["brov_coriolis_set", "brov_coriolis_off", "brov_coriolis_terms", "brov_coriolis_get", "brov_coriolis_eval_host",
           "brov_coriolis_last_host", "brov_coriolis_last_seconds"]
KERNELS = {"coriolis_eval_kernel": r"\d+coriolis_eval_kernelE", "plant_coriolis_kernel<0, 0>": r"\d+plant_coriolis_kernelILb0ELb0EE",
           "plant_coriolis_kernel<0, 1>": r"\d+plant_coriolis_kernelILb0ELb1EE", "plant_coriolis_kernel<1, 0>": r"\d+plant_coriolis_kernelILb1ELb0EE",
           "plant_coriolis_kernel<1, 1>": r"\d+plant_coriolis_kernelILb1ELb1EE"}
P_NOMINAL = np.array([0, 0, 0, 0, 1.7182, 0, 5.468, 0.4006, -11.7391, -20, -31.8678, -5, -18.18, -21.66, -36.99, -1.55])
U = 2.0 ** -53


def _lib():
    import bluerov2_amd
    from bluerov2_amd.solver import _load
    bluerov2_amd.build_library()
    return _load()


def test_header_declares_and_library_exports_exactly_the_seven_names():
    import bluerov2_amd
    bluerov2_amd.build_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(brov_coriolis_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(SYMBOLS), sorted(declared ^ set(SYMBOLS))
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("brov_coriolis_"))
    assert exported == set(SYMBOLS), sorted(exported ^ set(SYMBOLS))
    assert re.search(r"int\s+brov_coriolis_set\(brov_solver\* s, int terms\s*, double ka, double ma\);", txt)
    assert re.search(r"int\s+brov_coriolis_get\(const brov_solver\* s, int\* terms, double\* ka, double\* ma\);", txt)
    assert re.search(r"int\s+brov_coriolis_eval_host\(brov_solver\* s, const double\* x\s*, const double\* vc\s*, double\* c\s*\);", txt)
    assert dict(re.findall(r"#define (BROV_CORIOLIS_[A-Z_]+) (\d+)", txt)) == {"BROV_CORIOLIS_RIGID": "1", "BROV_CORIOLIS_ADDED": "2"}
    assert (bluerov2_amd.CORIOLIS_RIGID, bluerov2_amd.CORIOLIS_ADDED) == (1, 2) == (CO.RIGID, CO.ADDED)
    for name in ("set_coriolis", "coriolis_off", "coriolis_terms", "coriolis_eval", "coriolis_last", "coriolis_last_seconds"):
        assert callable(getattr(bluerov2_amd.BatchSolver, name)), name


def test_null_handles_are_argument_errors_with_the_calls_own_name():
    L = _lib()
    four = (ctypes.c_double * 12)()
    dp = ctypes.cast(four, ctypes.POINTER(ctypes.c_double))
    sec, ka, ma, terms = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int(7)
    calls = [("brov_coriolis_set", (None, 1, 0.0, 1.2481)), ("brov_coriolis_off", (None,)),
             ("brov_coriolis_get", (None, ctypes.byref(terms), ctypes.byref(ka), ctypes.byref(ma))), ("brov_coriolis_eval_host", (None, dp, None, dp)),
             ("brov_coriolis_last_host", (None, dp)), ("brov_coriolis_last_seconds", (None, ctypes.byref(sec)))]
    for name, args in calls:
        assert getattr(L, name)(*args) == ERR_ARG, (name, args)
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())   # the text of THIS call
    assert L.brov_coriolis_terms(None) == 0 and terms.value == 7


def test_new_kernels_use_no_scratch_and_the_makefile_gates_them():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "plant_coriolis.hip"], capture_output=True,
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
        assert hit[0]["VGPRs"] + hit[0]["AGPRs"] <= 256 and hit[0]["VGPRs"] <= 256 and hit[0]["occ"] >= 2, (short, hit[0])
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "plant_coriolis.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/plant_coriolis.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    assert "plant_coriolis_kernel" in rule and "coriolis_eval_kernel" in rule


# ---- the force against mechanics ----------------------------------------------------------------------------------------------------------------
def _skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def _points(n, seed):
    rng = np.random.default_rng(seed)
    nu = rng.normal(size=(n, 6)) * np.array([1.0, 1.0, 0.5, 0.5, 0.5, 1.0])
    nr = nu[:, :3] - rng.normal(size=(n, 3)) * 0.3
    added = rng.uniform(0.0, 8.0, (n, 3))
    return nu, nr, added, rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 2.0, n)


def test_the_force_is_rows_x_y_z_n_of_the_skew_matrix_form():
    """C(nu) = [[0, -S(M11 v1)], [-S(M11 v1), -S(M22 v2)]] for a diagonal M (Fossen 2011, eq. 6.43 with the CG at the origin; 6.54 for M_A),
    M11 = m I for the rigid body -- its M22 is left out: the angular rows of the model already carry (Iy - Iz) q r and the like, and the stage
    leaves the inertias the model's -- and M_A = diag(Xa, Ya, Za, ka, ma, .) at the velocity through the water.  200 random points, 1e-13
    relative to the largest term of the row."""
    nu, nr, added, ka, ma = _points(200, 31)
    worst = 0.0
    for i in range(len(nu)):
        v1, v2, v1r = nu[i, :3], nu[i, 3:], nr[i]
        Crb = np.zeros((6, 6)); Crb[:3, 3:] = -CO.MASS * _skew(v1); Crb[3:, :3] = -CO.MASS * _skew(v1)
        A11, A22 = np.diag(added[i]), np.diag([ka[i], ma[i], 0.0])
        Ca = np.zeros((6, 6)); Ca[:3, 3:] = -_skew(A11 @ v1r); Ca[3:, :3] = -_skew(A11 @ v1r); Ca[3:, 3:] = -_skew(A22 @ v2)
        rows = [0, 1, 2, 5]
        want_r = (-Crb @ nu[i])[rows]
        want_a = (-Ca @ np.concatenate([v1r, v2]))[rows]
        for terms, want in ((CO.RIGID, want_r), (CO.ADDED, want_a), (CO.RIGID | CO.ADDED, want_r + want_a)):
            got = CO.force(terms, nu[i], nr[i], added[i], ka[i], ma[i])
            scale = CO.MASS * np.abs(nu[i]).max() ** 2 + np.abs(added[i]).max() * max(np.abs(nu[i]).max(), np.abs(nr[i]).max()) ** 2
            worst = max(worst, np.abs(got - want).max() / scale)
    print(f"restated force against the skew-matrix form: worst relative difference {worst:.2e}")
    assert worst < 1e-13
    assert not CO.force(CO.RIGID, nu, nr, added)[:, 3].any()      # the rigid group leaves the yaw row to the model


def test_the_force_does_no_work():
    """-nu^T C(nu) nu = 0 for a skew-symmetric C: u cX + v cY + w cZ = 0 for the rigid group at any state; for the added group the three
    linear rows and the yaw row close among themselves whenever p = q = 0 (still water, so that the velocity through it is nu's own).  To
    rounding: each channel carries at most three roundings of its two terms, the power sum three more."""
    nu, _, added, ka, ma = _points(200, 32)
    c = CO.force(CO.RIGID, nu, nu[:, :3], added)
    power = nu[:, 0] * c[:, 0] + nu[:, 1] * c[:, 1] + nu[:, 2] * c[:, 2]
    scale = CO.MASS * 6.0 * np.abs(nu).max(axis=1) ** 3
    print(f"rigid group: worst |power| / scale = {np.abs(power / scale).max():.2e}")
    assert (np.abs(power) <= 8 * U * scale).all()
    flat = nu.copy(); flat[:, 3:5] = 0.0
    a = CO.force(CO.ADDED, flat, flat[:, :3], added, ka, ma)
    power = flat[:, 0] * a[:, 0] + flat[:, 1] * a[:, 1] + flat[:, 2] * a[:, 2] + flat[:, 5] * a[:, 3]
    scale = added.max(axis=1) * 6.0 * np.abs(flat).max(axis=1) ** 3
    print(f"added group, p = q = 0: worst |power| / scale = {np.abs(power / scale).max():.2e}")
    assert (np.abs(power) <= 8 * U * scale).all() and np.abs(a[:, :2]).min() > 0.0 and not a[:, 2].any()


def test_the_force_is_the_formulas_at_60_digits_to_four_roundings():
    """Every channel is a sum of products; a leaf product passes through at most four roundings on its way into the result (RIGID|ADDED, row X:
    Ya vr, (.) r, the difference, the add of the two groups; row N: Xa ur, (.) vr, the inner and the outer sum), each of relative size 2^-53:
    |restated - exact| <= 4 * 2^-53 * (sum of the magnitudes of the channel's leaf products).  The exact side is mpmath at 60 digits where it
    imports, as tests/model_exact.py's backend decides, else rational arithmetic."""
    be = model_exact.backend()
    if be.name == "mpmath":
        num, mass = be.num, be.num(CO.MASS)
    else:
        num, mass = (lambda v: Fraction(float(v))), Fraction(CO.MASS)
    nu, nr, added, ka, ma = _points(200, 33)
    worst = 0.0
    for i in range(len(nu)):
        u, v, w, p, q, r = (num(t) for t in nu[i])
        ur, vr, wr = (num(t) for t in nr[i])
        xa, ya, za, k, m = num(added[i, 0]), num(added[i, 1]), num(added[i, 2]), num(ka[i]), num(ma[i])
        leaf = {CO.RIGID: [[mass * r * v, -mass * q * w], [mass * p * w, -mass * r * u], [mass * q * u, -mass * p * v], []],
                CO.ADDED: [[ya * vr * r, -za * wr * q], [za * wr * p, -xa * ur * r], [xa * ur * q, -ya * vr * p],
                           [xa * ur * vr, -ya * vr * ur, k * p * q, -m * q * p]]}
        leaf[CO.RIGID | CO.ADDED] = [a + b for a, b in zip(leaf[CO.RIGID], leaf[CO.ADDED])]
        for terms, rows in leaf.items():
            got = CO.force(terms, nu[i], nr[i], added[i], ka[i], ma[i])
            for ch, terms_of_row in enumerate(rows):
                exact = sum(terms_of_row, num(0.0))
                bound = 4 * U * float(sum((abs(t) for t in terms_of_row), num(0.0)))
                err = abs(float(num(got[ch]) - exact))
                assert err <= bound, (i, terms, ch, err, bound)
                worst = max(worst, err / bound if bound else 0.0)
    print(f"restated force against {be.name if be.name == 'mpmath' else 'rational arithmetic'}: worst error {worst:.2f} of the bound")


def test_the_restated_sincos_is_a_sincos_and_the_projection_agrees_with_libm():
    """the bit-exact restatement of the device's sincos_pio2 (2 ulp, tests/test_gpu_model_exact.py) against libm, and water_velocity against
    x[6:9] - R^T vc with libm's R: nine entries of at most 3 ulp each times |vc| <= 1"""
    from wrench_restatement import rotation
    rng = np.random.default_rng(34)
    for a in np.concatenate([rng.uniform(-7.0, 7.0, 50), [0.0, -0.0, np.pi / 2, 300.0]]):
        s, c = CO.sincos_pio2(a)
        assert abs(s - np.sin(a)) <= 2 * np.spacing(1.0) and abs(c - np.cos(a)) <= 2 * np.spacing(1.0), a
    assert np.isnan(CO.sincos_pio2(np.nan)).all() and CO.fma(3.0, 5.0, -15.0) == 0.0 and CO.fma(1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0) == -2.0 ** -60
    for _ in range(20):
        x = rng.normal(size=12) * 0.5
        vc = rng.uniform(-0.5, 0.5, 3)
        assert np.abs(CO.water_velocity(x, vc) - (x[6:9] - rotation(x).T @ vc)).max() < 1e-15


def test_terms_zero_is_the_plant_in_moving_water_exactly(oracle):
    rng = np.random.default_rng(4)
    for substeps in (1, 4):
        x = rng.normal(size=12) * 0.2
        u, w, vc = rng.uniform(-5, 5, 4), rng.uniform(-20, 20, 6), rng.uniform(-0.4, 0.4, 3)
        p = P_NOMINAL.copy(); p[:4] = rng.uniform(-10, 10, 4)
        a = CO.rk4_under_coriolis(oracle, x, u, p, w, vc, 0, 0.05, substeps)
        assert np.array_equal(a, rk4_under_current(oracle, x, u, p, w, vc, 0.05, substeps))
        b = CO.rk4_under_coriolis(oracle, x, u, p, w, vc, CO.RIGID, 0.05, substeps)
        assert np.abs(a - b).max() > 1e-6
        # the stage touches rows 6, 7, 8, 11 alone, and the added group alone sees the current
        f0 = CO.f_under_coriolis(oracle, x, u, p, w, vc, 0)
        f3 = CO.f_under_coriolis(oracle, x, u, p, w, vc, CO.RIGID | CO.ADDED)
        assert np.array_equal(np.delete(f0, [6, 7, 8, 11]), np.delete(f3, [6, 7, 8, 11])) and np.abs(f0 - f3)[[6, 7, 8, 11]].min() > 1e-6
        still = np.zeros(3)
        assert not np.array_equal(CO.force(CO.ADDED, x[6:12], x[6:9], p[4:7]), CO.force(CO.ADDED, x[6:12], CO.water_velocity(x, vc), p[4:7]))
        assert np.array_equal(CO.water_velocity(x, still), x[6:9])


def test_the_phantom_disturbance_goes_with_the_rigid_body_terms(oracle):
    """The scenario of DESIGN.md section 4.9g on the CPU loop (scripts/coriolis_cpu_scenarios.py): circle, N = 20, B = 4, seed 21, level
    start, 80 ticks, no external disturbance, the observer's estimate handed to the controller; median |estimate| over the last 20 ticks.
    Measured: stage off 4.00 N on x and 12.36 N on y (the observer's model has the rigid-body products, the plant has not); RIGID 0.021 N and
    0.0045 N (190 x and 2700 x lower); yaw 0.014 N m under RIGID against 1.18 N m under RIGID|ADDED, which shows what the observer's model
    truly lacks."""
    N, B, ticks = 20, 4, 80
    traj, x0 = CO.scenario_inputs(B)
    pp = np.tile(P_NOMINAL, (B, 1))
    med = {}
    for terms in (0, CO.RIGID, CO.RIGID | CO.ADDED):
        log = CO.cpu_dob_loop(oracle, CO.ekf_for_the_device_plant(), terms, traj, x0, P_NOMINAL, pp, N, ticks)
        assert not log["status"].any() and np.isfinite(log["x"]).all()
        med[terms] = CO.phantom_medians(log["est"])
        print(f"terms {terms}: median |estimate| X {med[terms][0]:.4f} N, Y {med[terms][1]:.4f} N, N {med[terms][5]:.4f} N m")
    off, rigid, both = med[0], med[CO.RIGID], med[CO.RIGID | CO.ADDED]
    assert off[0] > 1.0 and off[1] > 1.0
    assert rigid[0] < 0.1 * off[0] and rigid[1] < 0.1 * off[1]
    assert both[5] > 10.0 * rigid[5]
