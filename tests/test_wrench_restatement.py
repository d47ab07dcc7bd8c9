"""The wrench generator's restatement (tests/wrench_restatement.py) against the properties include/bluerov2_nmpc.h states, and the
recorded-table fixture.  No GPU."""
import hashlib
import math
import os

import numpy as np

from wrench_restatement import WrenchRestatement, splitmix64_finalise, rotation, rk4_under_wrench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wrench_tables.npz")


def test_splitmix64_known_answers():
    """first outputs of SplitMix64 from state 0 and from 1234567 (the public-domain reference implementation's stream:
    state += golden gamma, output = finalise(state))"""
    g = 0x9E3779B97F4A7C15
    got = [int(splitmix64_finalise(np.uint64((k * g) & 0xFFFFFFFFFFFFFFFF))) for k in (1, 2, 3)]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    got = [int(splitmix64_finalise(np.uint64((1234567 + k * g) & 0xFFFFFFFFFFFFFFFF))) for k in (1, 2)]
    assert got == [6457827717110365317, 3203168211198807973]


def test_periodic_amplitudes_lie_in_3_6_and_are_redrawn_every_half_period():
    B = 64
    r = WrenchRestatement(B).periodic(seed=2024, dphi=0.125)
    ticks = 400                                            # t up to 50: 15 half periods
    A = np.stack([r.amplitudes(k) for k in range(ticks)])  # [ticks][B][4]
    assert A.min() >= 3.0 and A.max() < 6.0
    j = np.array([r.half_period(k) for k in range(ticks)])
    assert j[0] == 0 and j[-1] == int(math.floor(399 * 0.125 / math.pi)) and np.all(np.diff(j) >= 0)
    for k in range(1, ticks):
        same = np.array_equal(A[k], A[k - 1])
        assert same == (j[k] == j[k - 1]), k               # constant within a half period, redrawn -- every channel of every instance -- across
        if j[k] != j[k - 1]:
            assert np.all(A[k] != A[k - 1])
    # instances differ from each other, channels from each other
    assert len(np.unique(A[0][:, 0])) == B and len(np.unique(A[0][0])) == 4
    # another seed, another draw; the same seed, the same draw (no hidden state)
    assert np.all(WrenchRestatement(B).periodic(seed=2025).amplitudes(7) != A[7])
    assert np.array_equal(WrenchRestatement(B).periodic(seed=2024).amplitudes(7), A[7])
    # the draws fill the interval: mean of uniform[3, 6) within 5 standard errors
    a = A[::26].ravel()
    assert abs(a.mean() - 4.5) < 5 * (3 / math.sqrt(12)) / math.sqrt(a.size)


def test_periodic_wrench_shape_and_yaw_quirk():
    B = 32
    r = WrenchRestatement(B).periodic(seed=7, dphi=0.025, tz_div=3.0)     # the AMPC node's phase rate
    for k in (0, 1, 17, 125, 126, 999):
        w, A, sn = r.wrench(k), r.amplitudes(k), math.sin(0.0 + k * 0.025)
        assert np.array_equal(w[:, 0], sn * A[:, 0]) and np.array_equal(w[:, 1], sn * A[:, 1]) and np.array_equal(w[:, 2], sn * A[:, 2])
        assert not w[:, 3:5].any()
        assert np.array_equal(w[:, 5], w[:, 1] / 3.0)      # tz = fy / 3 bit for bit: the Y amplitude, not the N draw
    assert not r.wrench(0).any()                           # sin(0)
    # the phase is a product of the tick: any tick evaluates alone, in any order
    assert r.phase(1000) == 0.0 + 1000 * 0.025 and np.array_equal(r.wrench(999), WrenchRestatement(B).periodic(seed=7, dphi=0.025).wrench(999))


def test_constant_and_table_modes():
    B = 5
    c = WrenchRestatement(B).constant([10, 10, 10, 0, 0, 0])
    assert np.array_equal(c.wrench(0), np.tile([10.0, 10, 10, 0, 0, 0], (B, 1))) and np.array_equal(c.wrench(12345), c.wrench(0))
    tab = np.arange(18.0).reshape(3, 6)
    t = WrenchRestatement(B).table(tab)
    assert np.array_equal(t.wrench(1), np.tile(tab[1], (B, 1)))
    assert np.array_equal(t.wrench(2), t.wrench(3)) and np.array_equal(t.wrench(10 ** 9), np.tile(tab[2], (B, 1)))   # clamps at the end
    g = np.array([0.0, 0.5, 1.0, -2.0, 3.0])
    tg = WrenchRestatement(B).table(tab, gain=g)
    assert np.array_equal(tg.wrench(1), tab[1][None, :] * g[:, None])
    assert not WrenchRestatement(B).wrench(3).any()        # OFF


def test_table_fixture_digest_and_shape():
    g = np.load(GOLDEN)
    tab = g["table"]
    assert tab.shape == (496, 6) and tab.dtype == np.float64
    assert not tab[:, 3:5].any() and np.abs(tab[:, [0, 1, 2, 5]]).max() > 1.0
    assert hashlib.sha256(np.ascontiguousarray(tab).tobytes()).hexdigest() == str(g["table_sha256"])
    assert len(str(g["sha256"])) == 64
    # where the reference's recorded files are at hand (scripts/make_wrench_golden.py names the place), the fixture is checked against them
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import make_wrench_golden as mk
    cfg = os.path.join(mk.REFERENCE, "bluerov2_dobmpc", "config")
    if all(os.path.exists(os.path.join(cfg, f)) for f in mk.FILES):
        raw = [open(os.path.join(cfg, f), "rb").read() for f in mk.FILES]
        assert hashlib.sha256(b"".join(raw)).hexdigest() == str(g["sha256"])
        cols = [np.array([float(v) for v in r.split()]) for r in raw]
        assert np.array_equal(tab[:, [0, 1, 2, 5]], np.stack(cols, axis=1))
    # played back through the restatement: row k, then the last row for ever
    r = WrenchRestatement(2).table(tab)
    assert np.array_equal(r.wrench(100)[1], tab[100]) and np.array_equal(r.wrench(495), r.wrench(5000))


def test_plant_restatement_projects_the_wrench_per_stage(oracle):
    """level attitude: the world wrench is the body wrench (R = I at the start), and a zero wrench is the oracle's own RK4"""
    import bluerov2_amd as ba
    rng = np.random.default_rng(3)
    p = ba.P_NOMINAL.copy()
    x = np.zeros(12); x[2] = -20; x[6:] = rng.normal(size=6) * 0.1
    u = rng.uniform(-5, 5, 4)
    assert np.abs(rk4_under_wrench(oracle, x, u, p, np.zeros(6), 0.05) - oracle.rk4(x, u, p, 0.05)).max() < 1e-15
    # yawed by 90 degrees a world-x force pushes the body along -y
    xy = x.copy(); xy[5] = math.pi / 2
    R = rotation(xy)
    assert np.allclose(R.T @ np.array([1.0, 0, 0]), [0, -1, 0], atol=1e-15)
    # a wrench changes the step, and the per-stage projection differs from projecting once at the start when the vehicle turns
    xr = x.copy(); xr[3:6] = [0.3, -0.2, 1.0]; xr[11] = 0.8
    w = np.array([10.0, -6, 4, 0.5, -0.5, 2])
    a = rk4_under_wrench(oracle, xr, u, p, w, 0.05)
    Rr = rotation(xr)
    pb = p.copy(); fb, tb = Rr.T @ w[:3], Rr.T @ w[3:]
    pb[:3] += fb; pb[3] += tb[2]
    once = oracle.rk4(xr, u, pb, 0.05, drp=tb[:2])
    # (the attitude turns by |rates| h ~ 0.2 rad over the step at most, the wrench is ~12 N, the smallest inertia 0.3: the two differ by
    # less than h * 12 * 0.2 / 0.3 = 0.4, and by far more than rounding)
    assert 1e-9 < np.abs(a - once).max() < 0.4
