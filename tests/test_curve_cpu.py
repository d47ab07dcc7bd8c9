"""The plant's thrust-curve stage (brov_curve_*) without a GPU: the C ABI's symbols and declarations (include/bluerov2_nmpc_curve.h), the T200
fixture, tests/curve_restatement.py held to the header's text, the two pure helpers, the new kernels' resource report and the Makefile."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from curve_restatement import (BASIC, DEADZONE, LINEAR, PRE_NONE, PRE_POLY, PRE_TABLE, QNAN, TABLE, CurveRestatement, lookup, table_slopes)
from rotor_restatement import pinv_allocation

import bluerov2_amd as _ba

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
# the restatement speaks of the modes by the package's numbers
assert (LINEAR, BASIC, DEADZONE, TABLE) == (_ba.CURVE_LINEAR, _ba.CURVE_BASIC, _ba.CURVE_DEADZONE, _ba.CURVE_TABLE)
assert (PRE_NONE, PRE_POLY, PRE_TABLE) == (_ba.CURVE_PRE_NONE, _ba.CURVE_PRE_POLY, _ba.CURVE_PRE_TABLE)
SYMBOLS = ["brov_curve_default_params", "brov_curve_set_table_host", "brov_curve_get_table_host", "brov_curve_set_host", "brov_curve_off",
           "brov_curve_enabled", "brov_curve_reset", "brov_curve_eval_host", "brov_curve_last_host", "brov_curve_get_stats_host",
           "brov_curve_reset_stats", "brov_curve_last_seconds"]
KERNELS = {"command": r"curve_shift_kernelILi1E", "thrust": r"curve_shift_kernelILi2E", "both": r"curve_shift_kernelILi3E",
           "eval": r"\d+curve_eval_kernelE"}
LDS_STATED = 16384   # bytes: both tables at 256 knots, the amps column included


def _lib():
    import bluerov2_amd
    from bluerov2_amd.solver import _load
    bluerov2_amd.build_library()
    return _load()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def t200():
    """the fixture's columns and the curve table made of them (x = pwm - 1500), with the host's slopes; left unchanged"""
    import bluerov2_amd
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "t200_16v.json")))
    pwm, kgf, amps = (np.array(d[k], dtype=np.float64) for k in ("pwm", "kgf", "amps"))
    x, y, a = bluerov2_amd.curve_from_pwm_table(pwm, kgf, amps)
    tab = dict(x=x, y=y, slope=table_slopes(x, y), amps=a, amps_slope=table_slopes(x, a))
    for v in (pwm, kgf, amps, *tab.values()):
        v.setflags(write=False)
    return d, pwm, kgf, amps, tab


# ---- symbols ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_exactly_the_curve_names():
    import bluerov2_amd
    bluerov2_amd.build_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc_curve.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(brov_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(SYMBOLS), sorted(declared ^ set(SYMBOLS))
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("brov_curve_"))
    assert exported == set(SYMBOLS), sorted(exported ^ set(SYMBOLS))
    main = open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read()
    assert main.count('#include "bluerov2_nmpc_curve.h"') == 1
    assert main.index('#include "bluerov2_nmpc_curve.h"') > main.index('#include "bluerov2_nmpc_inspect.h"')
    assert "brov_curve_set_host" not in re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert "quadratic speed-to-thrust conversion" not in main                 # no longer out of the rotor stage's scope
    for name, val in (("LINEAR", 0), ("BASIC", 1), ("DEADZONE", 2), ("TABLE", 3), ("PRE_NONE", 0), ("PRE_POLY", 1), ("PRE_TABLE", 2),
                      ("PART_COMMAND", 1), ("PART_THRUST", 2), ("PART_BOTH", 3), ("WHICH_CURVE", 0), ("WHICH_PRE", 1), ("MAX_KNOTS", 256)):
        assert re.search(r"#define BROV_CURVE_%s %d\b" % (name, val), txt), name
        assert getattr(bluerov2_amd, "CURVE_" + name) == val
    body = re.search(r"typedef struct brov_curve_params \{(.*?)\} brov_curve_params;", txt, flags=re.S).group(1)
    fields = [tuple(d.split()) for d in body.split(";") if d.strip()]
    names = {ctypes.c_double: "double", ctypes.c_int32: "int32_t"}
    mirror = [(names[t._type_], "%s[%d]" % (n, t._length_)) if hasattr(t, "_length_") else (names[t], n) for n, t in bluerov2_amd.CurveParams._fields_]
    assert fields == mirror, fields
    p = bluerov2_amd.CurveParams.default()                                   # LINEAR, PRE_NONE, quantum 0: a copy
    assert (p.kind, p.pre, p.quantum, p.observer_applied) == (0, 0, 0.0, 0) and (p.k, p.kl, p.kr, p.dl, p.dr) == (1.0, 1.0, 1.0, 0.0, 0.0)
    assert list(p.pre_poly) == [0.0, 0.0, 0.0, 1.0, 0.0]


def test_null_handles_are_argument_errors_with_the_calls_own_name():
    L = _lib()
    buf = (ctypes.c_double * 256)()
    p = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))
    ibuf = (ctypes.c_int32 * 12)()
    ip = ctypes.cast(ibuf, ctypes.POINTER(ctypes.c_int32))
    steps = ctypes.c_int64(0)
    import bluerov2_amd
    par = bluerov2_amd.CurveParams.default()
    calls = [("brov_curve_set_table_host", (None, 0, p, p, None, 2)), ("brov_curve_get_table_host", (None, 0, p, p, p, p, p, ip)),
             ("brov_curve_set_host", (None, ctypes.byref(par), None)), ("brov_curve_off", (None,)), ("brov_curve_reset", (None,)),
             ("brov_curve_eval_host", (None, 3, p, p, p)), ("brov_curve_last_host", (None, p, p, p, p)),
             ("brov_curve_get_stats_host", (None, p, ip, p, ctypes.byref(steps))), ("brov_curve_reset_stats", (None,)),
             ("brov_curve_last_seconds", (None, p, p))]
    assert sorted(n for n, _ in calls) == sorted(set(SYMBOLS) - {"brov_curve_default_params", "brov_curve_enabled"})   # every entry point with a handle
    for name, args in calls:
        assert getattr(L, name)(*args) == ERR_ARG, (name, args)
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())   # the text of THIS call
    assert L.brov_curve_enabled(None) == 0
    L.brov_curve_default_params(None)                                         # tolerated


def test_python_names_exist():
    import bluerov2_amd
    for name in ("set_thrust_curve", "thrust_curve_off", "thrust_curve_enabled", "thrust_curve_reset", "thrust_curve_eval", "thrust_curve_last",
                 "thrust_curve_stats", "thrust_curve_table", "thrust_curve_last_seconds"):
        assert callable(getattr(bluerov2_amd.BatchSolver, name)), name
    for name in ("curve_from_pwm_table", "inverse_table", "CurveParams"):
        assert callable(getattr(bluerov2_amd, name)) and name in bluerov2_amd.__all__, name


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------------
def test_t200_fixture(t200):
    d, pwm, kgf, amps, tab = t200
    assert len(pwm) == len(kgf) == len(amps) == 201
    assert np.array_equal(pwm, 1100.0 + 4.0 * np.arange(201)) and pwm[-1] == 1900.0
    assert np.all(np.diff(kgf) >= 0.0)                                        # force non-decreasing
    band = (pwm >= 1472) & (pwm <= 1528)
    assert band.sum() == 15 and np.all(kgf[band] == 0.0) and np.all(kgf[~band] != 0.0)   # exactly the dead band
    assert kgf[0] == -4.07 and kgf[-1] == 5.25
    assert isinstance(d["voltage"], float) and d["voltage"] == 16.0           # one voltage
    assert np.all(amps >= 0.0) and np.all(amps[band] == 0.0) and amps[0] == 24.3
    assert set(d) == {"source", "voltage", "pwm", "kgf", "amps"}              # data only
    assert np.array_equal(tab["x"], pwm - 1500.0) and tab["x"][100] == 0.0 and tab["y"][100] == 0.0


# ---- the restatement, held to the header's text --------------------------------------------------------------------------------------------------
def _t200_stage(tab, B=1, **kw):
    return CurveRestatement(B, kind=TABLE, curve=tab, **kw)


def test_lookup_is_exact_on_every_knot_and_clamps_beyond_the_ends(t200):
    _, _, _, _, tab = t200
    x, y, s = tab["x"], tab["y"], tab["slope"]
    assert lookup(x, y, s, x).tobytes() == y.tobytes()                         # y[j] + slope[j] * 0
    assert lookup(x, tab["amps"], tab["amps_slope"], x).tobytes() == tab["amps"].tobytes()
    below = np.array([-np.inf, -1e300, -401.0, np.nextafter(-400.0, -np.inf), -400.0])
    above = np.array([np.inf, 1e300, 401.0, np.nextafter(400.0, np.inf), 400.0])
    assert np.all(lookup(x, y, s, below) == -4.07) and np.all(lookup(x, y, s, above) == 5.25)
    # between two knots: the chord, one rounding per operation
    w = np.array([-398.0, 30.0, 399.0, 5e-324])
    j = np.array([0, 107, 199, 100])
    assert np.array_equal(lookup(x, y, s, w), y[j] + s[j] * (w + (-x[j])))
    assert np.all(x[j] <= w) and np.all(w < x[j + 1])
    mid = 0.5 * (x[:-1] + x[1:])
    v = lookup(x, y, s, mid)
    assert np.all(v >= np.minimum(y[:-1], y[1:]) - 1e-15) and np.all(v <= np.maximum(y[:-1], y[1:]) + 1e-15)
    # two knots, the smallest table
    assert np.array_equal(lookup([0.0, 2.0], [1.0, 5.0], table_slopes([0.0, 2.0], [1.0, 5.0]), np.array([-1.0, 0.0, 0.5, 2.0, 3.0])),
                          [1.0, 1.0, 2.0, 5.0, 5.0])


def test_dead_band_gives_plus_zero_and_nan_passes(t200):
    _, _, _, _, tab = t200
    st = _t200_stage(tab)
    w = np.array([[-28.0, -27.999, -0.0, 0.0, 13.7, 28.0]])
    f, a = st.thrust(w)
    assert not f.any() and not np.signbit(f).any() and not a.any()              # +0.0 everywhere inside, and no current
    dz = CurveRestatement(1, kind=DEADZONE, kl=2.0, kr=3.0, dl=-4.0, dr=9.0)
    f, _ = dz.thrust(np.array([[-2.0, -0.0, 0.0, 2.9, 3.0, -3.0]]))            # v = -4, -0, 0, 8.41, 9, -9
    assert f.tobytes() == np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 2.0 * (-9.0 + 4.0)]]).tobytes()
    f, _ = dz.thrust(np.array([[4.0, -4.0, np.inf, -np.inf, 1e200, -1e200]]))
    assert np.array_equal(f, [[3.0 * 7.0, 2.0 * -12.0, np.inf, -np.inf, np.inf, -np.inf]])
    # a NaN passes every mode of both parts with its bits, whatever its payload and sign
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000123, 0xFFF0000000000001, 0x7FF4000000000000, 0x7FF8DEADBEEF0000],
                    dtype=np.uint64).view(np.float64).reshape(1, 6)
    pre = dict(x=tab["y"][[0, 50, 93, 107, 150, 200]], y=tab["x"][[0, 50, 93, 107, 150, 200]])
    pre["slope"] = table_slopes(pre["x"], pre["y"])
    for kind in (LINEAR, BASIC, DEADZONE, TABLE):
        for pre_mode in (PRE_NONE, PRE_POLY, PRE_TABLE):
            st = CurveRestatement(1, kind=kind, pre=pre_mode, quantum=4.0, k=0.5, eff=0.7, curve=tab, pre_table=pre, pre_poly=(1e-3, 0.0, 0.1, 9.7, 0.5))
            for part in ("command", "thrust", "both"):
                out, amps = st.eval(nans, part)
                assert out.tobytes() == nans.tobytes(), (kind, pre_mode, part)
                if kind == TABLE and part != "command":
                    assert amps.tobytes() == nans.tobytes()
    # a NaN the stage makes itself is the one quiet NaN: 0 * inf in BASIC with k = 0 and in the identity polynomial's leading zero
    f, _ = CurveRestatement(1, kind=BASIC, k=0.0).thrust(np.full((1, 6), np.inf))
    assert np.all(_bits(f) == _bits(QNAN))
    w = CurveRestatement(1, pre=PRE_POLY, pre_poly=(0.0, 0.0, 0.0, 1.0, 0.0)).command(np.full((1, 6), np.inf))
    assert np.all(_bits(w) == _bits(QNAN))


def test_quantisation_is_idempotent_and_ties_go_to_even():
    st = CurveRestatement(1, quantum=4.0)
    w = st.command(np.array([[2.0, 6.0, 10.0, -2.0, -6.0, 1.999]]))
    assert np.array_equal(w, [[0.0, 8.0, 8.0, -0.0, -8.0, 0.0]]) and np.signbit(w[0, 3])
    rng = np.random.default_rng(3)
    for q in (4.0, 0.1, 1.0 / 3.0, 1e-3, 7.0):
        st = CurveRestatement(500, quantum=q)
        t = rng.normal(size=(500, 6)) * 100.0
        w1 = st.command(t)
        assert st.command(w1).tobytes() == w1.tobytes(), q                      # a quantised command is a fixed point
        assert np.abs(w1 - t).max() <= 0.5 * q * (1.0 + 1e-12)
    st = CurveRestatement(1, quantum=4.0)
    big = st.command(np.array([[1e300, -1e300, np.inf, -np.inf, 5e-324, -5e-324]]))
    assert big.tobytes() == np.array([[1e300, -1e300, np.inf, -np.inf, 0.0, -0.0]]).tobytes()   # rint of a huge value is the value


def test_both_is_command_then_thrust_and_the_default_copies_the_record(t200):
    _, _, _, _, tab = t200
    B = 64
    rng = np.random.default_rng(4)
    pre = dict(x=np.array([-5.0, -1.0, 0.0, 2.0, 6.0]), y=np.array([-300.0, -40.0, 0.0, 60.0, 390.0]))
    pre["slope"] = table_slopes(pre["x"], pre["y"])
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e300, 5e-324])
    eff = rng.uniform(0.5, 1.5, (B, 6)); eff[::3] = 1.0
    for kind in (LINEAR, BASIC, DEADZONE, TABLE):
        for pre_mode in (PRE_NONE, PRE_POLY, PRE_TABLE):
            for q in (0.0, 4.0):
                kw = dict(kind=kind, pre=pre_mode, quantum=q, k=1e-4, kl=1e-4, kr=2e-4, dl=-100.0, dr=150.0, eff=eff, curve=tab, pre_table=pre,
                          pre_poly=(1e-4, 0.0, 0.01, 60.0, 1.0))
                one, two = CurveRestatement(B, **kw), CurveRestatement(B, **kw)
                for k in range(3):
                    t = rng.normal(size=(B, 6)) * 3.0
                    pick = rng.random((B, 6)) < 0.1
                    t[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
                    u0 = rng.normal(size=(B, 4))
                    bu, bt = one.step_both(u0, t, 0.05)
                    cu, ct = two.step_command(u0, t)
                    tu, tt = two.step_thrust(cu, ct, 0.05)
                    assert bu.tobytes() == tu.tobytes() and bt.tobytes() == tt.tobytes()
                    for name in ("wanted", "last_command", "last_thrust", "err_sq", "dead_ticks", "charge"):
                        assert getattr(one, name).tobytes() == getattr(two, name).tobytes(), name
                    # u0: the left inverse of what is delivered wherever a bit changed on the way, else the one received
                    changed = ((_bits(ct) != _bits(t)) | (_bits(tt) != _bits(ct))).any(axis=1)
                    with np.errstate(invalid="ignore", over="ignore"):
                        assert np.array_equal(_bits(bu), _bits(np.where(changed[:, None], pinv_allocation(bt), u0)))
                assert one.steps == 3
    # the default configuration copies the record, -0 and NaN included, and counts nothing but dead ticks of wanted zeros' complement
    st = CurveRestatement(2)
    t = np.array([[-0.0, 0.0, -0.0, 5.0, -7.0, np.nan], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]])
    u_in = np.array([[0.123, -0.0, 0.3, 1e-300], [9.0, 8.0, 7.0, 6.0]])
    u0, f = st.step_both(u_in, t, 0.05)
    assert f.tobytes() == t.tobytes() and u0.tobytes() == u_in.tobytes()
    assert st.err_sq[1] == 0.0 and not st.dead_ticks.any() and not st.charge.any()
    # an efficiency alone makes the record no copy: u0 is the left inverse of the delivered thrusts
    st = CurveRestatement(1, eff=[1.0, 1.0, 0.5, 1.0, 1.0, 1.0])
    u0, f = st.step_both(u_in[1:], t[1:], 0.05)
    assert np.array_equal(f, [[1.0, 2.0, 1.5, 4.0, 5.0, 6.0]]) and np.array_equal(u0, pinv_allocation(f)) and st.err_sq[0] == 1.5 ** 2


def test_books_count_dead_ticks_and_charge(t200):
    _, _, _, _, tab = t200
    st = _t200_stage(tab, B=1, quantum=4.0)
    t = np.array([[10.0, 0.0, -26.0, 30.0, 400.0, -400.0]])                    # 10 -> 8 and -26 -> -24: inside the band; 30 -> 32: outside
    for _ in range(3):
        _, f = st.step_both(np.zeros((1, 4)), t, 0.05)
    assert np.array_equal(st.dead_ticks, [[3, 0, 3, 0, 0, 0]]) and st.steps == 3
    assert f[0, 0] == 0.0 and f[0, 3] == 0.04 and f[0, 4] == 5.25 and f[0, 5] == -4.07
    amps = st.thrust(st.command(t))[1]
    assert amps[0, 4] == tab["amps"][-1] > 20.0 and amps[0, 5] == tab["amps"][0] == 24.3 and amps[0, 0] == 0.0
    s = amps[0, 0]
    for i in range(1, 6):
        s = s + amps[0, i]
    c = 0.0
    for _ in range(3):
        c = c + 0.05 * s
    assert st.charge[0] == c and c > 3 * 0.05 * 44.0


def test_curve_of_the_inverse_table_is_the_identity_within_one_table_step(t200):
    """inverse_table keeps 187 of the 201 knots: of the 15 of the dead band the first.  Outside the band the pre-map's output lies between
    the knots of the kept table that bracket the wanted thrust, and the curve is monotone, so curve(pre(t)) lies between their ordinates:
    within the largest ordinate step of the KEPT table of t.  That step is taken from the table here."""
    import bluerov2_amd
    _, _, _, _, tab = t200
    ix, iy = bluerov2_amd.inverse_table(tab["x"], tab["y"])
    assert len(ix) == 187 and np.all(np.diff(ix) > 0) and ix[0] == -4.07 and ix[-1] == 5.25
    assert iy[np.flatnonzero(ix == 0.0)[0]] == -28.0                           # of the dead band its FIRST knot: the lower edge
    assert not np.any((iy > -28.0) & (iy <= 28.0))                             # and none inside: the pre-map never asks for a dead command
    pre = dict(x=ix, y=iy, slope=table_slopes(ix, iy))
    st = CurveRestatement(1, kind=TABLE, pre=PRE_TABLE, curve=tab, pre_table=pre)
    step = np.diff(ix).max()                                                   # the largest force step between two kept knots
    assert 0.0 < step <= 0.2
    t = np.linspace(-4.07, 5.25, 6 * 4001).reshape(-1, 6)
    st.B = len(t); st.eff = np.ones((st.B, 6))
    f, _ = st.eval(t, "both")
    outside = np.abs(t) >= step                                                # wanted thrusts the band does not swallow
    print(f"largest kept step {step:.3f} kgf; worst |curve(pre(t)) - t| outside the band {np.abs(f - t)[outside].max():.3e}")
    assert np.all(np.abs(f - t)[outside] <= step)
    on_knots, _ = CurveRestatement(1, kind=TABLE, pre=PRE_TABLE, curve=tab, pre_table=pre).eval(np.resize(ix, (32, 6))[:1], "both")
    assert np.array_equal(on_knots[0], ix[:6])                                 # exact on the kept knots
    with pytest.raises(ValueError):
        bluerov2_amd.inverse_table([0.0, 1.0, 2.0], [1.0, 1.0, 1.0])
    x, y, a = bluerov2_amd.curve_from_pwm_table([1100.0, 1500.0, 1900.0], [-1.0, 0.0, 2.0], None, neutral=1500.0)
    assert np.array_equal(x, [-400.0, 0.0, 400.0]) and np.array_equal(y, [-1.0, 0.0, 2.0]) and a is None
    with pytest.raises(ValueError):
        bluerov2_amd.curve_from_pwm_table([1100.0, 1100.0], [0.0, 1.0])


# ---- resources -----------------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch_and_lds_within_the_stated_size():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "curve_kernel.hip"], capture_output=True,
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
        assert hit[0]["scratch"] == 0 and hit[0]["VGPRs Spill"] == 0 and hit[0]["lds"] == 0, (short, hit[0])   # the tables' LDS is dynamic
        assert hit[0]["VGPRs"] <= 128 and hit[0]["occ"] >= 4, (short, hit[0])
    assert len(rep) == 4, sorted(rep)
    # the dynamic request: the images of both tables at 256 knots, the stated 16 KiB; the formula is the header's, restated
    src = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "nmpc_device.hpp")).read()
    assert "((K + 1) & ~1) + 2 * K + (amps ? 2 * K : 0)" in src

    def doubles(K, amps):
        return ((K + 1) & ~1) + 2 * K + (2 * K if amps else 0)
    assert 8 * (doubles(256, True) + doubles(256, False)) == LDS_STATED
    assert doubles(201, True) % 2 == 0 and doubles(201, False) % 2 == 0      # every image and every part of one starts on 16 bytes
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "curve_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/curve_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    assert "curve_shift_kernel" in rule and "curve_eval_kernel" in rule
