"""CPU restatement of the sensor stage (include/bluerov2_nmpc.h, brov_sensor_*), the yardstick of sensor_measure_kernel and sensor_eval_kernel
in bluerov2_amd/csrc/sensor_kernel.hip.  A helper, not collected.

Fresh sample of channel c of instance b at measurement index m, x the true value:
    v = (x + bias[b][c]) + sigma[b][c] * n(b, m, c)
    y = quant[c] > 0 ? rint(v / quant[c]) * quant[c] : v
every operation one IEEE FP64 operation in this order: numpy elementwise `*`, `+`, `/` are separate operations and never contract; np.rint
rounds ties to even.  The noise is built from integers alone:
    H(k) = splitmix64_finalise((seed ^ 0x53454E534F52) + (k + 1) * 0x9E3779B97F4A7C15),   k = b << 32 | m << 8 | c << 2 | j
    S = the sum of the twelve 16-bit fields of H at j = 0, 1, 2;   n = (S - 393210) / 65536          (exact; Irwin-Hall(12), unit variance)
and the dropout draw of (b, m) is u = (H >> 11) * 2^-53 at the channel slot c = 12, j = 0: dropped iff dropout[b] > 0 and u < dropout[b].
Regular refresh at m: a dropped fix samples nothing; otherwise channel c is sampled iff m % period[c] == 0, else held.  Then dropped += drop and
err_sq[b][c] += d * d with d = y[c] - x[c] after the refresh.  Forced refresh: every channel sampled, no draw, no statistic."""
import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SALT = 0x53454E534F52
MAX_INDEX = 1 << 24


def finalise(z):
    """SplitMix64's output function on a Python integer"""
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def _finalise_u64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hashes(seed, b, m, c, j):
    """H(k) for arrays b, m, c (broadcast against each other) and the scalar j, as uint64 (array arithmetic wraps modulo 2^64)"""
    b, m, c = (np.asarray(v).astype(np.uint64) for v in (b, m, c))
    k = np.atleast_1d((b << np.uint64(32)) | (m << np.uint64(8)) | (c << np.uint64(2)) | np.uint64(j))   # (scalars would warn on overflow)
    base = np.array([(int(seed) ^ SALT) & MASK64], dtype=np.uint64)
    return _finalise_u64(base + (k + np.uint64(1)) * np.uint64(GOLDEN))


def noise(seed, b, m, c):
    """n(b, m, c), float64, exact"""
    S = 0
    for j in range(3):
        h = hashes(seed, b, m, c, j)
        for sh in (0, 16, 32, 48):
            S = S + ((h >> np.uint64(sh)) & np.uint64(0xFFFF)).astype(np.int64)
    return (S - 393210).astype(np.float64) / 65536.0


def dropout_draw(seed, b, m):
    """u(b, m) in [0, 1), float64, exact"""
    return (hashes(seed, b, m, 12, 0) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


class SensorRestatement:
    def __init__(self, B, seed=0, sigma=None, bias=None, quant=None, period=None, dropout=None):
        self.B, self.seed = int(B), int(seed)
        self.sigma = np.broadcast_to(np.asarray(0.0 if sigma is None else sigma, dtype=np.float64), (self.B, 12)).copy()
        self.bias = np.broadcast_to(np.asarray(0.0 if bias is None else bias, dtype=np.float64), (self.B, 12)).copy()
        self.quant = np.broadcast_to(np.asarray(0.0 if quant is None else quant, dtype=np.float64), (12,)).copy()
        self.period = np.broadcast_to(np.asarray(1 if period is None else period, dtype=np.int64), (12,)).copy()
        self.dropout = np.broadcast_to(np.asarray(0.0 if dropout is None else dropout, dtype=np.float64), (self.B,)).copy()
        self.y = np.zeros((self.B, 12))
        self.reset_stats()

    def reset_stats(self):
        self.dropped = np.zeros(self.B, dtype=np.int32)
        self.err_sq = np.zeros((self.B, 12))
        self.refreshes = 0

    def sample(self, m, x):
        """fresh samples [B][12] of the states x at index m; moves nothing"""
        assert 0 <= int(m) < MAX_INDEX
        x = np.asarray(x, dtype=np.float64)
        n = noise(self.seed, np.arange(self.B)[:, None], int(m), np.arange(12)[None, :])
        with np.errstate(invalid="ignore", over="ignore"):
            v = x + self.bias
            v = v + self.sigma * n
            q = np.where(self.quant > 0.0, self.quant, 1.0)
            r = np.rint(v / q)
            return np.where(self.quant > 0.0, r * q, v)

    def verdict(self, m):
        """[B] bool: is the fix of index m dropped?"""
        assert 0 <= int(m) < MAX_INDEX
        return (self.dropout > 0.0) & (dropout_draw(self.seed, np.arange(self.B), int(m)) < self.dropout)

    def forced(self, m, x):
        self.y = self.sample(m, x)
        return self.y

    def refresh(self, m, x):
        """the regular refresh behind a plant step; returns the verdicts"""
        x = np.asarray(x, dtype=np.float64)
        drop = self.verdict(m)
        take = (~drop)[:, None] & ((int(m) % self.period) == 0)[None, :]
        self.y = np.where(take, self.sample(m, x), self.y)
        self.dropped = self.dropped + drop.astype(np.int32)
        with np.errstate(invalid="ignore", over="ignore"):
            d = self.y - x
            self.err_sq = self.err_sq + d * d
        self.refreshes += 1
        return drop


def same(a, b):
    """equal values, NaNs compared by position"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan], b[~nan])


def same_stats(st, r):
    return np.array_equal(st["dropped"], r.dropped) and same(st["err_sq"], r.err_sq) and st["refreshes"] == r.refreshes
