"""CPU restatement of the plant's ocean current (include/bluerov2_nmpc.h, brov_current_*; the constant_current block of the reference's
underwater_current_plugin, bluerov2_environ/worlds/ocean_waves.world), the yardstick of bluerov2_amd/csrc/plant_current.hip.  A helper,
not collected.

Generator: every operation one IEEE FP64 operation in the order the header states it (numpy elementwise arithmetic never contracts into
FMAs); the 64-bit mixing in np.uint64, which wraps around.  Constant and table mode are pure functions of (data, instance, tick); the
Gauss-Markov mode holds the state c [B][3], which a plant step at tick k applies as it stands and then advances:
    U  = (splitmix64_finalise(seed + (n + 1) * GOLDEN_GAMMA) >> 11) * 2^-53,  n = (b << 24) | (k << 2) | i
    xi = 2 U - 1
    v  = (c[i] - step * (mu[i] * (c[i] - mean[b][i]))) + amp[i] * xi
    c[i] = v < lo[i] ? lo[i] : (v > hi[i] ? hi[i] : v)

Model: the current vc is a world-frame water velocity.  f_under_current takes f_under_wrench at x and replaces its rows 6..8 by rows 6..8
of the same call at x with x[6:9] - R^T vc.  Exact for this model: rows 6..8 see the linear velocities only through the two damping
terms, and no other row is touched.  RK4, the plant step and a DOB loop on top, as tests/wrench_restatement.py builds them."""
import numpy as np

from wrench_restatement import GOLDEN_GAMMA, f_under_wrench, rotation, splitmix64_finalise

OFF, CONSTANT, TABLE, GAUSS_MARKOV = 0, 1, 2, 3

# The Gauss-Markov case of tests/test_gpu_current.py (B = 96, 64 plant steps from tick GM_TICK0): the instances' means are spread beyond both
# bounds, so that some states sit at a bound throughout, some wander into one and some never meet one (tests/test_current_cpu.py checks that
# states clamp on either side and that some never do).
GM_CASE = dict(seed=0x5EA0CEA0C0FFEE01, mu=[0.5, 0.8, 0.3], amp=[0.02, 0.012, 0.008], lo=[-0.20, -0.10, -0.05], hi=[0.30, 0.20, 0.04], step=0.05)
GM_TICK0, GM_STEPS = 1000, 64


def gm_case_mean(B):
    return np.random.default_rng(77).uniform(-0.5, 0.6, (B, 3)) * np.array([1.0, 0.5, 0.2])


def current_from_angles(speed, horizontal, vertical):
    """the plugin's convention: (V cos h cos v, V sin h cos v, V sin v)"""
    return np.array([speed * np.cos(horizontal) * np.cos(vertical), speed * np.sin(horizontal) * np.cos(vertical), speed * np.sin(vertical)])


class CurrentRestatement:
    def __init__(self, B):
        self.B = int(B)
        self.mode = OFF
        self.last = np.zeros((self.B, 3))
        self.clamped_lo = np.zeros((self.B, 3), dtype=np.int64)   # how often a state was clamped at either bound: a property of the inputs
        self.clamped_hi = np.zeros((self.B, 3), dtype=np.int64)

    def constant(self, v):
        self.v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.B, 3)))
        self.mode = CONSTANT
        return self

    def table(self, tab, gain=None):
        self.tab = np.ascontiguousarray(tab, dtype=np.float64)
        assert self.tab.ndim == 2 and self.tab.shape[1] == 3
        self.gain = None if gain is None else np.asarray(gain, dtype=np.float64).reshape(self.B)
        self.mode = TABLE
        return self

    def gauss_markov(self, seed, mean, mu, amp, lo=None, hi=None, step=0.05):
        three = lambda v, d: np.broadcast_to(np.asarray(d if v is None else v, dtype=np.float64), (3,)).copy()
        self.seed = np.uint64(seed)
        self.mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (self.B, 3)).copy()
        self.mu, self.amp, self.lo, self.hi, self.tick_seconds = three(mu, 0), three(amp, 0), three(lo, -5.0), three(hi, 5.0), float(step)
        self.c = self.mean.copy()                                  # entering the mode sets the state to the mean
        self.mode = GAUSS_MARKOV
        return self

    def set_state(self, c):
        assert self.mode == GAUSS_MARKOV
        self.c = np.broadcast_to(np.asarray(c, dtype=np.float64), (self.B, 3)).copy()

    def current(self, k):
        """[B][3] the constant / table current at tick k (zeros while off)"""
        assert self.mode != GAUSS_MARKOV, "a state, not a function of the tick"
        if self.mode == OFF:
            return np.zeros((self.B, 3))
        if self.mode == CONSTANT:
            return self.v.copy()
        row = self.tab[min(max(int(k), 0), self.tab.shape[0] - 1)]
        g = np.ones(self.B) if self.gain is None else self.gain
        return row[None, :] * g[:, None]

    def state(self, k):
        """what a plant step at tick k applies"""
        return self.c.copy() if self.mode == GAUSS_MARKOV else self.current(k)

    def uniform(self, k):
        """[B][3] the draws of tick k: 53 bits of one SplitMix64 output each"""
        assert 0 <= int(k) < 2 ** 22
        b = np.arange(self.B, dtype=np.uint64)[:, None]
        i = np.arange(3, dtype=np.uint64)[None, :]
        n = (b << np.uint64(24)) | (np.uint64(k) << np.uint64(2)) | i
        with np.errstate(over="ignore"):
            z = splitmix64_finalise(self.seed + (n + np.uint64(1)) * GOLDEN_GAMMA)
        return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53

    def advance(self, k):
        xi = 2.0 * self.uniform(k)
        xi = xi - 1.0
        d = self.c - self.mean
        d = self.mu * d
        d = self.tick_seconds * d
        v = self.c - d
        n = self.amp * xi
        v = v + n
        self.clamped_lo += v < self.lo
        self.clamped_hi += v > self.hi
        self.c = np.where(v < self.lo, self.lo, np.where(v > self.hi, self.hi, v))

    def step(self, k):
        """the current a plant step at tick k applies; Gauss-Markov mode: the state then moves on"""
        vc = self.state(k)
        self.last = vc.copy()
        if self.mode == GAUSS_MARKOV:
            self.advance(k)
        return vc


def f_under_current(oracle, x, u, p, w, vc, drp=None):
    """the oracle's model under the world wrench w[6] in water that moves with the world-frame velocity vc[3]"""
    x = np.asarray(x, dtype=np.float64)
    f = np.array(f_under_wrench(oracle, x, u, p, w, drp), dtype=np.float64, copy=True)
    xr = x.copy()
    xr[6:9] = x[6:9] - rotation(x).T @ np.asarray(vc, dtype=np.float64)
    f[6:9] = np.asarray(f_under_wrench(oracle, xr, u, p, w, drp))[6:9]
    return f


def rk4_under_current(oracle, x, u, p, w, vc, dt, substeps=1, drp=None):
    """one control period of the plant: `substeps` ERK4 steps, wrench and current held, projected afresh at every stage"""
    x = np.array(x, dtype=np.float64, copy=True)
    h = dt / substeps
    for _ in range(substeps):
        k1 = f_under_current(oracle, x, u, p, w, vc, drp)
        k2 = f_under_current(oracle, x + 0.5 * h * k1, u, p, w, vc, drp)
        k3 = f_under_current(oracle, x + 0.5 * h * k2, u, p, w, vc, drp)
        k4 = f_under_current(oracle, x + h * k3, u, p, w, vc, drp)
        x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return x


def plant_step(oracle, x, u, p, w, vc, dt=0.05, substeps=1, g=None):
    """batched: x [B][12], u [B][4], p [B][16], w [B][6] or None, vc [B][3].  g [B][6]: the step behind the thruster stage, the way
    thruster_restatement.plant_step poses it: the input is zero, the stage's forces enter as disturbances and its roll / pitch moments
    as the 6-disturbance variant's"""
    B = len(x)
    w = np.zeros((B, 6)) if w is None else w
    out = []
    for b in range(B):
        if g is None:
            out.append(rk4_under_current(oracle, x[b], u[b], p[b], w[b], vc[b], dt, substeps))
            continue
        pa = np.array(p[b], dtype=np.float64, copy=True)
        pa[0] += g[b, 0]; pa[1] += g[b, 1]; pa[2] += g[b, 2]; pa[3] += g[b, 5]
        out.append(rk4_under_current(oracle, x[b], np.zeros(4), pa, w[b], vc[b], dt, substeps, drp=np.array([g[b, 3], g[b, 4]])))
    return np.stack(out)


def cpu_dob_loop(oracle, ekf, current, traj, x0, p_ctrl, p_true, N, ticks, line0=0, dt=0.05, substeps=1, handoff=True, Ts=None):
    """wrench_restatement.cpu_dob_loop in moving water: window(line0 + k) -> the oracle's RTI step -> the restated plant under
    current.step(k) -> the oracle EKF fed with the new plant state, the thrust allocation of the applied input and (v - v_prev) / dt ->
    p[0..3] of every stage := the EKF's hand-off (skipped with handoff=False: the uncompensated controller; ekf=None: no observer at all).
    Returns dict(u [ticks][B][4], x [ticks+1][B][12], status [ticks][B], current [ticks][B][3], est [ticks][B][6])."""
    from oracle import trajectory_oracle as T
    B = len(x0)
    op = oracle.opts(N, Ts)
    x, u, pi, lam = oracle.init_iterate(op, B)
    pfull = np.ascontiguousarray(np.broadcast_to(np.asarray(p_ctrl, dtype=np.float64).reshape(-1, 16)[:, None, :], (B, N + 1, 16)))
    xe, Pe = ekf.init_state(B) if ekf is not None else (None, None)
    xc = np.array(x0, dtype=np.float64, copy=True)
    vprev = np.zeros((B, 6))
    rotor = 0.026546960744430276
    log = dict(u=[], x=[xc.copy()], status=[], current=[], est=[])
    res = None
    for k in range(ticks):
        yref = np.ascontiguousarray(np.broadcast_to(T.window(traj, line0 + k, N), (B, N + 1, 16)))
        _, res = oracle.rti_step_batch(op, xc, yref, pfull, x, u, pi, lam, res_prev=res)
        u0 = res["u0"].copy()
        vc = current.step(k)
        xc = plant_step(oracle, xc, u0, p_true, None, vc, dt, substeps)
        log["u"].append(u0); log["x"].append(xc.copy()); log["status"].append(res["status"].copy()); log["current"].append(vc)
        if ekf is None:
            continue
        t = np.stack([(-u0[:, 0] + u0[:, 1] + u0[:, 3]), (-u0[:, 0] - u0[:, 1] - u0[:, 3]), (u0[:, 0] + u0[:, 1] - u0[:, 3]),
                      (u0[:, 0] - u0[:, 1] + u0[:, 3]), -u0[:, 2], -u0[:, 2]], axis=1) / rotor
        acc = (xc[:, 6:12] - vprev) / ekf.par.dt
        vprev = xc[:, 6:12].copy()
        _, mp, rc = ekf.update(xe, Pe, t, xc, acc)
        assert rc == 0
        if handoff:
            pfull[:, :, :4] = mp[:, None, :]
        log["est"].append(xe[:, 12:].copy())
    return {k: np.array(v) for k, v in log.items()}
