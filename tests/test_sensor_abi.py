"""The sensor stage (brov_sensor_*) without a GPU: the C ABI's symbols and declarations, the argument checks that need no device, the
BatchSolver methods, the new kernels' resource report and the Makefile's gate, the counter hash against published answers, the statistics of
the noise variate, and the numpy restatement against answers worked by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np

import sensor_restatement as SR
from sensor_restatement import SensorRestatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SYMBOLS = ["brov_sensor_set_host", "brov_sensor_off", "brov_sensor_enabled", "brov_sensor_measure", "brov_sensor_eval_host",
           "brov_sensor_get_measurement_host", "brov_sensor_get_stats_host", "brov_sensor_reset_stats", "brov_sensor_last_seconds"]
KERNELS = {"sensor_measure_kernel": r"\d+sensor_measure_kernelE", "sensor_eval_kernel": r"\d+sensor_eval_kernelE"}


def _lib():
    import bluerov2_amd
    from bluerov2_amd.solver import _load
    bluerov2_amd.build_library()
    return _load()


def test_header_declares_and_library_exports_exactly_the_sensor_names():
    import bluerov2_amd
    bluerov2_amd.build_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(brov_sensor_[a-z0-9_]+)\s*\(", txt))
    assert declared == set(SYMBOLS), sorted(declared ^ set(SYMBOLS))
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("brov_sensor_"))
    assert exported == set(SYMBOLS), sorted(exported ^ set(SYMBOLS))
    assert re.search(r"int\s+brov_sensor_set_host\(brov_solver\* s, uint64_t seed, const double\* sigma\s*, const double\* bias\s*,\s*"
                     r"const double\* quant\s*, const int32_t\* period\s*, const double\* dropout\s*\);", txt)
    assert re.search(r"int\s+brov_sensor_eval_host\(brov_solver\* s, int64_t index, const double\* x\s*, double\* y\s*, int32_t\* dropped\s*\);", txt)


def test_null_handles_are_argument_errors_with_the_calls_own_name():
    L = _lib()
    buf = (ctypes.c_double * 12)()
    p12 = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))
    sec = ctypes.c_double(0.0)
    calls = [("brov_sensor_set_host", (None, 0, None, None, None, None, None)), ("brov_sensor_off", (None,)), ("brov_sensor_measure", (None, None)),
             ("brov_sensor_eval_host", (None, 0, p12, p12, None)), ("brov_sensor_get_measurement_host", (None, p12)),
             ("brov_sensor_get_stats_host", (None, None, None, None)), ("brov_sensor_reset_stats", (None,)),
             ("brov_sensor_last_seconds", (None, ctypes.byref(sec)))]
    for name, args in calls:
        assert getattr(L, name)(*args) == ERR_ARG, (name, args)
        assert L.brov_last_error().decode().startswith(name + ":"), (name, L.brov_last_error())   # the text of THIS call
    assert L.brov_sensor_enabled(None) == 0


def test_batch_solver_methods_exist():
    import bluerov2_amd
    for name in ("set_sensors", "sensors_off", "sensors_enabled", "sensor_measure", "sensor_eval", "measured_state", "sensor_stats",
                 "sensor_reset_stats", "sensor_last_seconds"):
        assert callable(getattr(bluerov2_amd.BatchSolver, name)), name


def test_new_kernels_use_no_scratch_and_the_makefile_gates_them():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "sensor_kernel.hip"], capture_output=True,
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
    assert "sensor_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/sensor_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    assert "sensor_measure_kernel" in rule and "sensor_eval_kernel" in rule


def test_hash_known_answers():
    """the first two outputs of SplitMix64 from seed 0 (the published sequence): the finaliser over the first two multiples of the increment"""
    g = SR.GOLDEN
    assert SR.finalise(g) == 0xE220A8397B1DCDAF
    assert SR.finalise((2 * g) % 2 ** 64) == 0x6E789E6AA1B965F4
    # the array form is the same function, and H(k) is it over (seed ^ salt) + (k + 1) * increment
    z = np.array([g, (2 * g) % 2 ** 64, 12345], dtype=np.uint64)
    assert [int(v) for v in SR._finalise_u64(z)] == [SR.finalise(int(v)) for v in z]
    b, m, c, j, seed = 3, 77, 5, 2, 0xDEADBEEF
    k = (b << 32) | (m << 8) | (c << 2) | j
    assert int(SR.hashes(seed, b, m, c, j)[0]) == SR.finalise(((seed ^ 0x53454E534F52) + (k + 1) * g) % 2 ** 64)


def test_noise_statistics():
    """n over b < 4096, m < 64, c < 12 with seed 7: 3.1 M Irwin-Hall(12) variates.  The bounds are five standard errors of each estimator
    (mean: 5 / sqrt(N) = 0.0028; variance: 5 sqrt(1.9 / N) = 0.0039; kurtosis: about 0.012; a correlation over N / 12 ... N pairs: < 0.01)."""
    n = SR.noise(7, np.arange(4096)[:, None, None], np.arange(64)[None, :, None], np.arange(12)[None, None, :])
    assert n.shape == (4096, 64, 12)
    s = n * 65536.0
    assert np.array_equal(s, np.rint(s))                       # every n is a multiple of 2^-16
    mean, var = n.mean(), n.var()
    kurt = ((n - mean) ** 4).mean() / var ** 2
    print(f"mean {mean:.4f}, variance {var:.5f}, kurtosis {kurt:.4f}, max |n| {np.abs(n).max():.2f}")
    assert abs(mean) < 0.003 and abs(var - 1.0) < 0.004
    assert abs(kurt - 2.9) < 0.02 and np.abs(n).max() <= 6.0

    def corr(a, b):
        return abs(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    worst = max(corr(n[:, :, a], n[:, :, b]) for a in range(12) for b in range(a + 1, 12))
    lag_m, lag_b = corr(n[:, :-1], n[:, 1:]), corr(n[:-1], n[1:])
    print(f"correlations: channel pairs <= {worst:.4f}, tick lag 1 {lag_m:.4f}, instance lag 1 {lag_b:.4f}")
    assert worst < 0.01 and lag_m < 0.01 and lag_b < 0.01
    # the dropout draw is uniform on [0, 1)
    u = SR.dropout_draw(7, np.arange(4096)[:, None], np.arange(64)[None, :])
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / u.size)


def test_restatement_has_the_answers_worked_by_hand():
    """Two instances, sigma = 0, dyadic numbers: every rounded operation is exact and the literals are the hand computation.  Instance 1 drops
    every fix (dropout 1: u < 1 always); channel 1 has period 3; channel 2 is quantised to 0.25."""
    x = np.zeros((2, 12)); x[:, 0] = 1.0; x[:, 1] = 2.0; x[:, 2] = 0.625
    bias = np.zeros(12); bias[0] = 0.5
    quant = np.zeros(12); quant[2] = 0.25
    period = np.ones(12, dtype=int); period[1] = 3
    r = SensorRestatement(2, seed=9, bias=bias, quant=quant, period=period, dropout=[0.0, 1.0])
    # sigma = 0: the sample is x + bias; 0.625 / 0.25 = 2.5 is a tie and goes to the even 2 -> 0.5
    y = r.sample(0, x)
    assert np.array_equal(y[:, :3], [[1.5, 2.0, 0.5]] * 2) and not y[:, 3:].any()
    x2 = x.copy(); x2[:, 2] = 0.875                                  # 3.5 is a tie too and goes to the even 4 -> 1.0
    assert np.array_equal(r.sample(5, x2)[:, 2], [1.0, 1.0])
    x2[:, 2] = 0.8125                                                # 3.25 -> 3 -> 0.75
    assert np.array_equal(r.sample(5, x2)[:, 2], [0.75, 0.75])
    assert r.refreshes == 0 and not r.dropped.any() and not r.err_sq.any() and not r.y.any()      # evaluation moves nothing
    # a forced refresh ignores period and dropout and touches no statistic
    assert np.array_equal(r.forced(1, x)[:, :3], [[1.5, 2.0, 0.5]] * 2)
    assert r.refreshes == 0 and not r.dropped.any() and not r.err_sq.any()
    # the plant moves: x0 -> 3, x1 -> 4.  Regular refreshes at 1, 2 (channel 1 holds), 3 (channel 1 samples); instance 1 holds everything
    xm = x.copy(); xm[:, 0] = 3.0; xm[:, 1] = 4.0
    for m, y1 in ((1, 2.0), (2, 2.0), (3, 4.0)):
        drop = r.refresh(m, xm)
        assert np.array_equal(drop, [False, True])
        assert np.array_equal(r.y[0, :3], [3.5, y1, 0.5]) and np.array_equal(r.y[1, :3], [1.5, 2.0, 0.5])
    assert np.array_equal(r.dropped, [0, 3]) and r.refreshes == 3
    # err_sq: instance 0: channel 0 the bias, 3 x 0.5^2; channel 1 two held ticks, 2 x 2^2; channel 2 (0.5 - 0.625)^2 x 3
    # instance 1 (everything held at the forced sample): channel 0 3 x 1.5^2, channel 1 3 x 2^2, channel 2 as above
    assert np.array_equal(r.err_sq[0, :3], [0.75, 8.0, 3 * 0.015625]) and np.array_equal(r.err_sq[1, :3], [6.75, 12.0, 3 * 0.015625])
    assert not r.err_sq[:, 3:].any()
    # a NaN state gives a NaN measurement, quantised or not, and only there; zeros keep their value
    xn = x.copy(); xn[0, 2] = np.nan; xn[1, 5] = np.nan; xn[0, 7] = -0.0
    yn = r.sample(4, xn)
    assert np.isnan(yn[0, 2]) and np.isnan(yn[1, 5]) and np.isnan(yn).sum() == 2 and yn[0, 7] == 0.0
    # indices are 24 bits
    for bad in (-1, 1 << 24):
        try:
            r.sample(bad, x)
        except AssertionError:
            continue
        raise AssertionError(bad)
