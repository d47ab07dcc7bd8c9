"""CPU restatement of the plant's Coriolis stage (include/bluerov2_nmpc.h, brov_coriolis_*; the rigid-body products of BLUEROV2_DOB::f(),
bluerov2_dobmpc/src/bluerov2_dob.cpp:651-677, and the C_RB + C_A of dynamics_C(), :894-906), the yardstick of
bluerov2_amd/csrc/plant_coriolis.hip.  A helper, not collected.

Force: rows X, Y, Z, N of -C_RB(nu) nu and -C_A(nu_r) nu_r, every product and every difference one IEEE FP64 operation in the order the
header states it (numpy elementwise arithmetic never contracts into FMAs):
    RIGID (1)  cX = m ((r v) - (q w))     cY = m ((p w) - (r u))     cZ = m ((q u) - (p v))     cN = 0
    ADDED (2)  ax = Xa ur, ay = Ya vr, az = Za wr;  bx = ka p, by = ma q
               aX = (ay r) - (az q)       aY = (az p) - (ax r)       aZ = (ax q) - (ay p)       aN = ((ax vr) - (ay ur)) + ((bx q) - (by p))
    both (3)   one add per channel, rigid + added

water_velocity: what the device's evaluation kernel (and the `last` rows of the plant kernel) give the added-mass group in moving water,
x[6:9] - R^T vc with R from the device's own sincos (sincos_pio2 of bluerov2_model.hpp: its fused multiply-adds restated exactly in
rational arithmetic, rounded once), every product and sum rounded on its own, the sums left to right.

Model: f_under_coriolis is current_restatement.f_under_current with p[0..3] of the call raised by the force at that point -- exact, since
the terms enter where the disturbances do; the added-mass group sees x[6:9] - R^T vc (libm's R here, as f_under_current has it).  RK4, the
plant step and a DOB loop on top, as tests/current_restatement.py builds them."""
from fractions import Fraction

import numpy as np

from current_restatement import f_under_current
from wrench_restatement import rotation

RIGID, ADDED = 1, 2
MASS = 11.26
MA_REFERENCE = 1.2481          # added_mass[4] of the reference; added_mass[3] = 0


def force(terms, nu, nr, added, ka=0.0, ma=MA_REFERENCE):
    """[..., 4] = [X Y Z N] at nu [..., 6] = (u v w p q r), the velocity through the water nr [..., 3] and added [..., 3] = (Xa, Ya, Za)"""
    nu, nr, added = (np.asarray(a, dtype=np.float64) for a in (nu, nr, added))
    u, v, w, p, q, r = (nu[..., i] for i in range(6))
    ur, vr, wr = (nr[..., i] for i in range(3))
    zero = np.zeros(np.broadcast(u, ur, added[..., 0]).shape)
    g = [zero, zero, zero, zero]
    a = [zero, zero, zero, zero]
    with np.errstate(all="ignore"):
        if terms & RIGID:
            t0 = r * v; t1 = q * w; g0 = MASS * (t0 - t1)
            t0 = p * w; t1 = r * u; g1 = MASS * (t0 - t1)
            t0 = q * u; t1 = p * v; g2 = MASS * (t0 - t1)
            g = [g0, g1, g2, zero]
        if terms & ADDED:
            ax = added[..., 0] * ur; ay = added[..., 1] * vr; az = added[..., 2] * wr
            bx = ka * p; by = ma * q
            t0 = ay * r; t1 = az * q; a0 = t0 - t1
            t0 = az * p; t1 = ax * r; a1 = t0 - t1
            t0 = ax * q; t1 = ay * p; a2 = t0 - t1
            t0 = ax * vr; t1 = ay * ur; d0 = t0 - t1
            t0 = bx * q; t1 = by * p; d1 = t0 - t1
            a = [a0, a1, a2, d0 + d1]
        if (terms & RIGID) and (terms & ADDED):
            out = [gi + ai for gi, ai in zip(g, a)]
        else:
            out = a if terms & ADDED else g
    return np.stack([np.broadcast_to(o, zero.shape) for o in out], axis=-1).astype(np.float64)


# ---- the device's sincos, bit for bit ---------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """a * b + c rounded once"""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        return a * b + c          # the sign of a zero: as the sum of the (here exact or zero) product and c
    return float(exact)           # int / int true division: correctly rounded


def sincos_pio2(a):
    """(sin a, cos a) as sincos_pio2 of bluerov2_model.hpp computes them, operation for operation"""
    a = float(a)
    if not np.isfinite(a):
        return float("nan"), float("nan")
    n = float(np.rint(np.float64(a) * np.float64(6.36619772367581382433e-01)))
    r = fma(-n, 1.57079632679489655800e+00, a)
    r = fma(-n, 6.12323399573676603587e-17, r)
    r = fma(-n, -1.49738490485916983e-33, r)
    z = r * r
    ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08)
    ps = fma(z, ps, 2.75573137070700676789e-06)
    ps = fma(z, ps, -1.98412698298579493134e-04)
    ps = fma(z, ps, 8.33333333332248946124e-03)
    ps = fma(z, ps, -1.66666666666666324348e-01)
    s = fma(r * z, ps, r)
    pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09)
    pc = fma(z, pc, -2.75573143513906633035e-07)
    pc = fma(z, pc, 2.48015872894767294178e-05)
    pc = fma(z, pc, -1.38888888888741095749e-03)
    pc = fma(z, pc, 4.16666666666666019037e-02)
    c = fma(z * z, pc, fma(z, -0.5, 1.0))
    q = int(n) & 3
    s1, c1 = (c, s) if q & 1 else (s, c)
    return (-s1 if q & 2 else s1), (-c1 if (q + 1) & 2 else c1)


def water_velocity(x, vc):
    """[3] = x[6:9] - R^T vc as the device's water_velocity (plant_stages.hpp) rounds it"""
    x, vc = np.asarray(x, dtype=np.float64), np.asarray(vc, dtype=np.float64)
    (sph, cph), (sth, cth), (sps, cps) = (tuple(np.float64(t) for t in sincos_pio2(x[i])) for i in (3, 4, 5))
    with np.errstate(all="ignore"):
        t = cps * sth; r01 = t * sph - sps * cph
        t = cps * cph; r02 = sps * sph + t * sth
        t = sph * sth; r11 = cps * cph + t * sps
        t = sth * sps; r12 = t * cph - cps * sph
        r00, r10, r20, r21, r22 = cps * cth, sps * cth, -sth, cth * sph, cth * cph
        out = []
        for i, (ra, rb, rc) in enumerate(((r00, r10, r20), (r01, r11, r21), (r02, r12, r22))):
            acc = ra * vc[0] + rb * vc[1]
            acc = acc + rc * vc[2]
            out.append(x[6 + i] - acc)
    return np.array(out, dtype=np.float64)


def force_at(terms, x, p, vc=None, ka=0.0, ma=MA_REFERENCE):
    """batched: what brov_coriolis_eval_host returns for the states x [B][12], the plant parameters p [B][16] and the water velocities
    vc [B][3] (None: still water, the velocity through the water IS x[6:9])"""
    x, p = np.asarray(x, dtype=np.float64), np.asarray(p, dtype=np.float64)
    nr = x[:, 6:9] if vc is None else np.stack([water_velocity(x[b], vc[b]) for b in range(len(x))])
    return force(terms, x[:, 6:12], nr, p[:, 4:7], ka, ma)


# ---- the model under the stage ----------------------------------------------------------------------------------------------------------------
def f_under_coriolis(oracle, x, u, p, w, vc, terms, ka=0.0, ma=MA_REFERENCE, drp=None):
    """the oracle's model under the world wrench w[6] in water moving with vc[3], with the stage's force on top"""
    x, p = np.asarray(x, dtype=np.float64), np.asarray(p, dtype=np.float64)
    vc = np.zeros(3) if vc is None else np.asarray(vc, dtype=np.float64)
    if not terms:
        return f_under_current(oracle, x, u, p, w, vc, drp)
    nr = x[6:9] - rotation(x).T @ vc
    pa = p.copy()
    pa[:4] = pa[:4] + force(terms, x[6:12], nr, p[4:7], ka, ma)
    return f_under_current(oracle, x, u, pa, w, vc, drp)


def rk4_under_coriolis(oracle, x, u, p, w, vc, terms, dt, substeps=1, ka=0.0, ma=MA_REFERENCE, drp=None):
    """one control period of the plant: `substeps` ERK4 steps, wrench and current held, the force evaluated afresh at every stage"""
    x = np.array(x, dtype=np.float64, copy=True)
    h = dt / substeps
    f = lambda y: f_under_coriolis(oracle, y, u, p, w, vc, terms, ka, ma, drp)
    for _ in range(substeps):
        k1 = f(x)
        k2 = f(x + 0.5 * h * k1)
        k3 = f(x + 0.5 * h * k2)
        k4 = f(x + h * k3)
        x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return x


def plant_step(oracle, x, u, p, w, vc, terms, dt=0.05, substeps=1, ka=0.0, ma=MA_REFERENCE, g=None):
    """batched: x [B][12], u [B][4], p [B][16], w [B][6] or None, vc [B][3] or None.  g [B][6]: the step behind the thruster stage, as
    current_restatement.plant_step poses it: the input is zero, the stage's forces enter as disturbances and its roll / pitch moments as the
    6-disturbance variant's"""
    B = len(x)
    w = np.zeros((B, 6)) if w is None else w
    vc = np.zeros((B, 3)) if vc is None else vc
    out = []
    for b in range(B):
        if g is None:
            out.append(rk4_under_coriolis(oracle, x[b], u[b], p[b], w[b], vc[b], terms, dt, substeps, ka, ma))
            continue
        pa = np.array(p[b], dtype=np.float64, copy=True)
        pa[0] += g[b, 0]; pa[1] += g[b, 1]; pa[2] += g[b, 2]; pa[3] += g[b, 5]
        out.append(rk4_under_coriolis(oracle, x[b], np.zeros(4), pa, w[b], vc[b], terms, dt, substeps, ka, ma, drp=np.array([g[b, 3], g[b, 4]])))
    return np.stack(out)


def cpu_dob_loop(oracle, ekf, terms, traj, x0, p_ctrl, p_true, N, ticks, ka=0.0, ma=MA_REFERENCE, line0=0, dt=0.05, substeps=1, handoff=True, Ts=None):
    """wrench_restatement.cpu_dob_loop with the plant under the stage and no external disturbance: window(line0 + k) -> the oracle's RTI
    step -> the restated plant -> the oracle EKF fed with the new plant state, the thrust allocation of the applied input and
    (v - v_prev) / dt -> p[0..3] of every stage := the EKF's hand-off.  Returns dict(u [ticks][B][4], x [ticks+1][B][12], status [ticks][B],
    est [ticks][B][6])."""
    from oracle import trajectory_oracle as T
    B = len(x0)
    op = oracle.opts(N, Ts)
    x, u, pi, lam = oracle.init_iterate(op, B)
    pfull = np.ascontiguousarray(np.broadcast_to(np.asarray(p_ctrl, dtype=np.float64).reshape(-1, 16)[:, None, :], (B, N + 1, 16)))
    xe, Pe = ekf.init_state(B)
    xc = np.array(x0, dtype=np.float64, copy=True)
    vprev = np.zeros((B, 6))
    rotor = 0.026546960744430276
    log = dict(u=[], x=[xc.copy()], status=[], est=[])
    res = None
    for k in range(ticks):
        yref = np.ascontiguousarray(np.broadcast_to(T.window(traj, line0 + k, N), (B, N + 1, 16)))
        _, res = oracle.rti_step_batch(op, xc, yref, pfull, x, u, pi, lam, res_prev=res)
        u0 = res["u0"].copy()
        xc = plant_step(oracle, xc, u0, p_true, None, None, terms, dt, substeps, ka, ma)
        log["u"].append(u0); log["x"].append(xc.copy()); log["status"].append(res["status"].copy())
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


def phantom_medians(est, last=20):
    """[6]: the median |estimate| per channel (X Y Z K M N) over the last `last` ticks and the batch"""
    e = np.abs(np.asarray(est)[-last:])
    return np.median(e.reshape(-1, e.shape[-1]), axis=0)


def scenario_inputs(B=4, seed=21):
    """the scenario of DESIGN.md section 4.9g: the circle from a level start, B = 4, seed 21"""
    from oracle import trajectory_oracle as T
    rng = np.random.default_rng(seed)
    traj = T.circle()
    x0 = np.zeros((B, 12)); x0[:, :6] = traj[0, :6]; x0[:, :3] += rng.normal(size=(B, 3)) * 0.05
    return traj, x0


def ekf_for_the_device_plant():
    """the oracle EKF configured as tests/test_gpu_plant_wrench.py::_ekf_pair configures it"""
    from oracle.oracle_ffi import EkfOracle
    e = EkfOracle(); e.par.compensate_coef = 1.0; e.par.rotor_constant = 1.0
    for j in range(12, 24):
        e.par.K[j] = 0.0
    return e
