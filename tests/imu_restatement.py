"""The IMU/GPS stage of the solver's plant (include/bluerov2_nmpc_imu.h, brov_imu_*) in numpy: the yardstick of tests/test_imu_cpu.py,
tests/test_gpu_imu.py and tests/test_gpu_eskf_rates_loop.py.  Written from the formulas of the header, not from the kernel.  The noise is the
sensor stage's counter-based variate (tests/sensor_restatement.py: hashes, noise) at the channel slots 16..28; the geometry is that of
tests/eskf_exact.py (np_inputs_from_state).  What is bit for bit on the device: the flags, and the sums (noiseless + bias) + sigma * n."""
import numpy as np

import eskf_exact as X
from sensor_restatement import MAX_INDEX, hashes, noise

SLOT_ACC, SLOT_GYRO, SLOT_GPS, SLOT_ATT, SLOT_DROP = 16, 19, 22, 25, 28
GPSV_ELAPSED = 1


def dropout_draw(seed, b, m):
    """u(b, m) in [0, 1) of the IMU stage: slot 28, j = 0"""
    return (hashes(seed, b, m, SLOT_DROP, 0) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def channel_noise(seed, B, m, slot, n):
    """[B][n]: n(b, m, slot + k)"""
    return noise(seed, np.arange(B)[:, None], int(m), slot + np.arange(n)[None, :])


class ImuRestatement:
    def __init__(self, B, h, gps_every=1, seed=0, sigma=None, bias=None, dropout=None, g=9.81, flags=0):
        self.B, self.h, self.g, self.gps_every, self.seed, self.flags = int(B), float(h), float(g), int(gps_every), int(seed), int(flags)
        self.sigma = np.broadcast_to(np.asarray(0.0 if sigma is None else sigma, dtype=np.float64), (self.B, 12)).copy()
        self.bias = np.broadcast_to(np.asarray(0.0 if bias is None else bias, dtype=np.float64), (self.B, 6)).copy()
        self.dropout = np.broadcast_to(np.asarray(0.0 if dropout is None else dropout, dtype=np.float64), (self.B,)).copy()
        self.v_prev, self.p_last, self.m_last = np.zeros((self.B, 3)), np.zeros((self.B, 3)), np.zeros(self.B, dtype=np.int64)
        self.imu, self.gps_p, self.gps_v, self.q_meas = np.zeros((self.B, 6)), np.zeros((self.B, 3)), np.zeros((self.B, 3)), np.zeros((self.B, 4))
        self.fix = np.zeros(self.B, dtype=np.int32)
        self.reset_stats()

    def reset_stats(self):
        self.samples, self.fixes, self.dropped = (np.zeros(self.B, dtype=np.int32) for _ in range(3))

    def due(self, m):
        return int(m) % self.gps_every == 0

    def verdict(self, m):
        """[B] bool: is a fix due at index m dropped?"""
        return (self.dropout > 0.0) & (dropout_draw(self.seed, np.arange(self.B), int(m)) < self.dropout)

    def flags_at(self, m):
        """[B] int32: fix[b] of a regular refresh at index m"""
        return (self.due(m) & ~self.verdict(m)).astype(np.int32) if self.due(m) else np.zeros(self.B, dtype=np.int32)

    def sample(self, m, x, v_prev, p_last, m_last, forced=False):
        """the stage alone; returns dict(imu, gps_p, gps_v, q_meas, fix, v_I); without a fix the GPS entries are zeros"""
        assert 0 <= int(m) < MAX_INDEX
        x = np.asarray(x, dtype=np.float64)
        B = self.B
        na, nw = channel_noise(self.seed, B, m, SLOT_ACC, 3), channel_noise(self.seed, B, m, SLOT_GYRO, 3)
        npos, natt = channel_noise(self.seed, B, m, SLOT_GPS, 3), channel_noise(self.seed, B, m, SLOT_ATT, 3)
        fix = np.ones(B, dtype=np.int32) if forced else self.flags_at(m)
        o = dict(imu=np.zeros((B, 6)), gps_p=np.zeros((B, 3)), gps_v=np.zeros((B, 3)), q_meas=np.zeros((B, 4)), fix=fix, v_I=np.zeros((B, 3)))
        for b in range(B):
            ph, th, ps = x[b, 3:6]
            R = X.np_rot_euler(ph, th, ps)
            vI = R @ x[b, 6:9]
            vp = vI if forced else v_prev[b]
            a = R.T @ ((vI - vp) / self.h - np.array([0.0, 0.0, -self.g]))
            o["imu"][b, 0:3] = (a + self.bias[b, 0:3]) + self.sigma[b, 0:3] * na[b]
            o["imu"][b, 3:6] = (x[b, 9:12] + self.bias[b, 3:6]) + self.sigma[b, 3:6] * nw[b]
            o["v_I"][b] = vI
            if not fix[b]:
                continue
            gp = x[b, 0:3] + self.sigma[b, 6:9] * npos[b]
            if forced or m_last[b] < 0:
                gv = np.zeros(3)
            else:
                steps = (int(m) - int(m_last[b])) if self.flags & GPSV_ELAPSED else self.gps_every
                gv = (gp - p_last[b]) / (float(steps) * self.h)
            c, s = np.cos, np.sin
            q = np.array([c(ps / 2) * c(th / 2) * c(ph / 2) + s(ps / 2) * s(th / 2) * s(ph / 2), c(ps / 2) * c(th / 2) * s(ph / 2) - s(ps / 2) * s(th / 2) * c(ph / 2),
                          c(ps / 2) * s(th / 2) * c(ph / 2) + s(ps / 2) * c(th / 2) * s(ph / 2), s(ps / 2) * c(th / 2) * c(ph / 2) - c(ps / 2) * s(th / 2) * s(ph / 2)])
            o["gps_p"][b], o["gps_v"][b] = gp, gv
            o["q_meas"][b] = X.np_unit(X.np_qmul(q, X.np_exp(self.sigma[b, 9:12] * natt[b])))
        return o

    def _take(self, m, o):
        f = o["fix"].astype(bool)
        self.imu, self.fix, self.v_prev = o["imu"], o["fix"], o["v_I"]
        for name in ("gps_p", "gps_v", "q_meas"):
            getattr(self, name)[f] = o[name][f]
        self.p_last[f] = o["gps_p"][f]
        self.m_last[f] = int(m)

    def restart(self, m, x):
        """the forced restart: gravity alone, a fix without a dropout draw, gps_v = 0; no statistic"""
        self._take(m, self.sample(m, x, None, None, None, forced=True))

    def refresh(self, m, x):
        """the regular refresh behind a plant step; returns the flags"""
        o = self.sample(m, x, self.v_prev, self.p_last, self.m_last)
        self._take(m, o)
        self.samples += 1
        self.fixes += o["fix"]
        if self.due(m):
            self.dropped += self.verdict(m).astype(np.int32)
        return o["fix"]
