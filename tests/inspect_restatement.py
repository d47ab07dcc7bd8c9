"""The range stage and the inspection controller (include/bluerov2_nmpc_inspect.h, brov_range_*, brov_inspect_*) in numpy and plain Python
floats: the yardstick of tests/test_inspect_cpu.py and tests/test_gpu_inspect.py, and what scripts/inspect_cpu_scenarios.py flies.  Written
from the formulas of the header and from reading the reference's VisualController, not from the kernel.  Every operation here is one IEEE
double operation, as on the device, so the rays, the tree sum and the controller are bit for bit; the rotation is taken as an argument (the
device's own in the GPU tests, rot_np here), because sines and cosines of two libraries differ in the last place."""
import math

import numpy as np

from bluerov2_amd.inspect import INSPECT_FLOAT_YAW, INSPECT_SHARED_PID
from bluerov2_amd.solver import RESULT_DTYPE, ROTOR_CONSTANT
from sensor_restatement import MAX_INDEX, noise  # noqa: F401

SLOT_RANGE = 32
TWO_PI, HALF_PI = 2 * math.pi, 0.5 * math.pi


# ---- the rotation ----------------------------------------------------------------------------------------------------------------------
def rot_np(phi, theta, psi):
    """[9], row-major: the model body's rotation from numpy's sines and cosines"""
    sph, cph, sth, cth, sps, cps = np.sin(phi), np.cos(phi), np.sin(theta), np.cos(theta), np.sin(psi), np.cos(psi)
    return np.array([cps * cth, (cps * sth) * sph - sps * cph, sps * sph + (cps * cph) * sth,
                     sps * cth, cps * cph + (sph * sth) * sps, (sth * sps) * cph - cps * sph,
                     -sth, cth * sph, cth * cph])


def rot_mp(phi, theta, psi, digits=60):
    """the same rotation in `digits`-digit arithmetic: a list of 9 mpmath numbers"""
    import mpmath as mp
    with mp.workdps(digits):
        a, b, c = mp.mpf(float(phi)), mp.mpf(float(theta)), mp.mpf(float(psi))
        sph, cph, sth, cth, sps, cps = mp.sin(a), mp.cos(a), mp.sin(b), mp.cos(b), mp.sin(c), mp.cos(c)
        return [cps * cth, cps * sth * sph - sps * cph, sps * sph + cps * cph * sth,
                sps * cth, cps * cph + sph * sth * sps, sth * sps * cph - cps * sph,
                -sth, cth * sph, cth * cph]


def rot_error(rot, phi, theta, psi):
    """scaled error of a double rotation [9] against the 60-digit one: max |got - ref| / max(1, |ref|) = max |got - ref|"""
    import mpmath as mp
    ref = rot_mp(phi, theta, psi)
    with mp.workdps(60):
        return float(max(abs(mp.mpf(float(g)) - r) for g, r in zip(rot, ref)))


# ---- the rays ----------------------------------------------------------------------------------------------------------------------------
def cast(rot, p, cam, lo, hi):
    """one instance: (range without noise, hits, depth [roi * roi] with 0.0 for no return) for the rotation rot [9], the position p [3], the
    camera cam (RangeParams) and the boxes lo, hi [K, 3]"""
    R = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1, 3), np.asarray(hi, dtype=np.float64).reshape(-1, 3)
    roi, half = int(cam.roi), int(cam.roi) // 2
    q = np.arange(roi * roi)
    j = q // roi
    i = q - j * roi
    a = (((i - half) + 0.5) - cam.cx) / cam.f
    b = (((j - half) + 0.5) - cam.cy) / cam.f
    m = [cam.mount[0], cam.mount[1], cam.mount[2]]
    o = [p[c] + ((R[c, 0] * m[0] + R[c, 1] * m[1]) + R[c, 2] * m[2]) for c in range(3)]
    inf = np.inf
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = [1.0 / ((R[c, 0] + R[c, 1] * (-a)) + R[c, 2] * (-b)) for c in range(3)]
        best = np.full(q.shape, inf)
        for k in range(len(lo)):
            tn, tf = np.full(q.shape, -inf), np.full(q.shape, inf)
            for c in range(3):
                t1, t2 = (lo[k, c] - o[c]) * inv[c], (hi[k, c] - o[c]) * inv[c]
                tn = np.fmax(tn, np.fmin(t1, t2))
                tf = np.fmin(tf, np.fmax(t1, t2))
            hit = (tn <= tf) & (tn >= cam.near) & (tn <= cam.far) & (tn < best)
            best = np.where(hit, tn, best)
        ret = best < inf
        rng = np.where(ret, best, 0.0) * np.sqrt((1.0 + a * a) + b * b)
    # lane l takes the rays l, l + 64, ... in that order; then the fixed tree
    pad = (-len(q)) % 64
    rr = np.concatenate([rng, np.zeros(pad)]).reshape(-1, 64)
    hh = np.concatenate([ret, np.zeros(pad, dtype=bool)]).reshape(-1, 64)
    s, n = np.zeros(64), np.zeros(64, dtype=np.int64)
    for row in range(len(rr)):
        s = np.where(hh[row], s + rr[row], s)
        n = n + hh[row]
    stride = 32
    while stride >= 1:
        s[:stride] = s[:stride] + s[stride:2 * stride]
        n[:stride] = n[:stride] + n[stride:2 * stride]
        stride //= 2
    return (s[0] / n[0] if n[0] > 0 else 0.0), int(n[0]), np.where(ret, best, 0.0)


def range_eval(rot, x, cam, lo, hi, sigma=None, m=0):
    """the batch: dict(range [B] with the noise, hits [B], depth [B, roi * roi]) for rot [B, 9] and the states x [B, 12] at index m"""
    B = len(x)
    out = dict(range=np.zeros(B), hits=np.zeros(B, dtype=np.int32), depth=np.zeros((B, int(cam.roi) ** 2)))
    sg = np.broadcast_to(np.asarray(0.0 if sigma is None else sigma, dtype=np.float64), (B,))
    nz = noise(int(cam.seed), np.arange(B), int(m), SLOT_RANGE)
    for b in range(B):
        r, n, d = cast(rot[b], x[b, :3], cam, lo, hi)
        out["range"][b] = r + sg[b] * nz[b] if n > 0 else 0.0
        out["hits"][b], out["depth"][b] = n, d
    return out


# ---- the controller --------------------------------------------------------------------------------------------------------------------------
def _pid(par, s, loop, ref, pos):
    a = 0 if par.flags & INSPECT_SHARED_PID else loop
    e = ref - pos
    integral = float(s["integral"][a]) + e * par.dt
    d = (e - float(s["prev_error"][a])) / par.dt
    out = (par.gains[loop * 3] * e + par.gains[loop * 3 + 1] * integral) + par.gains[loop * 3 + 2] * d
    s["integral"][a], s["prev_error"][a] = integral, e
    return out


def control(par, s, t, rng, z, psi):
    """one tick of one instance: the state record s (INSPECT_STATE_DTYPE) and the statistics record t (or None) move in place; returns the
    result record (RESULT_DTYPE) and whether the "state machine failed" branch was taken"""
    fl = bool(par.flags & INSPECT_FLOAT_YAW)
    F = (lambda v: float(np.float32(v))) if fl else (lambda v: float(v))
    rng, z, psi = float(rng), float(z), float(psi)
    k = int(s["k"])
    s["k"] = k + 1
    if t is not None and rng != 0.0 and (t["min_range"] == 0.0 or rng < t["min_range"]):
        t["min_range"] = rng
    if rng > par.buffer:
        s["started"] = 1
    c1 = c2 = c3 = c4 = 0.0
    failed = False
    if s["started"]:
        yaw, pre = math.remainder(psi, TWO_PI), float(s["pre_yaw"])
        if pre >= 0.0 and yaw >= 0.0:
            diff = F(yaw - pre)
        elif pre >= 0.0 and yaw < 0.0:
            wrap, direct = (TWO_PI + yaw) - pre, pre + abs(yaw)
            diff = F(-direct) if wrap >= direct else F(wrap)
        elif pre < 0.0 and yaw >= 0.0:
            wrap, direct = (TWO_PI - yaw) + pre, abs(pre) + yaw
            diff = F(direct) if wrap >= direct else F(-wrap)
        else:
            diff = F(yaw - pre)
        s["yaw_sum"] = F(float(s["yaw_sum"]) + diff)
        s["pre_yaw"] = F(yaw)
        ysum = float(s["yaw_sum"])
        lo, hi = par.safety_dis - par.buffer, par.safety_dis + par.buffer
        in_band = lo <= rng <= hi
        turned, rounded = bool(s["completed_turn"]), bool(s["completed_round"])

        def zyaw():
            return _pid(par, s, 1, float(s["ref_z"]), z), _pid(par, s, 2, float(s["ref_yaw"]), ysum)
        if k * par.dt < par.t_hold:
            c1 = _pid(par, s, 0, par.safety_dis, rng)
            c3 = _pid(par, s, 1, par.z0, z)
            c4 = _pid(par, s, 2, par.yaw0, ysum)
        elif not s["completed_mission"]:
            if in_band and turned and not rounded:
                s["status"], s["ref_x"] = 0, par.safety_dis
                c1 = _pid(par, s, 0, float(s["ref_x"]), rng)
                c3, c4 = zyaw()
                c2 = par.sway
                s["completed_turn"], s["turn"], s["get_height"] = 1, 0, 1
            elif rng > hi and turned:
                s["status"] = 1
                c3, c4 = zyaw()
                c2 = par.sway_slow
            elif rng < par.lost and not s["turn"]:
                s["completed_turn"], s["status"] = 0, 2
                s["ref_yaw"] = float(s["ref_yaw"]) + HALF_PI
                c3, c4 = zyaw()
                s["turn"] = 1
            elif s["turn"] and not turned:
                s["status"] = 2
                c3, c4 = zyaw()
                if abs(float(s["ref_yaw"]) - ysum) < par.yaw_tol:
                    s["completed_turn"] = 1
                    if abs(yaw - par.yaw0) < par.yaw_home_tol:
                        s["completed_round"] = 1
                        s["cycle_counter"] += 1
                        if t is not None:
                            t["rounds"] += 1
                        if abs(float(s["ref_z"]) - F(par.z_goal)) < par.height_tol:
                            s["completed_mission"] = 1
                    else:
                        s["completed_round"] = 0
            elif rng < par.lost and turned:
                s["status"] = 3
                c1, c2 = par.surge_search, par.sway
                c3, c4 = zyaw()
            elif in_band and turned and rounded:
                s["status"] = 4
                if s["get_height"]:
                    s["ref_z"] = float(s["ref_z"]) + par.dz_round
                    s["ref_x"] = par.safety_dis
                    c3, c4 = zyaw()
                    s["get_height"] = 0
                else:
                    s["ref_x"] = par.safety_dis
                    c3, c4 = zyaw()
                    if abs(float(s["ref_z"]) - z) < par.z_tol:
                        s["completed_round"] = 0
            else:
                failed = True
                s["status"] = 2
                c3, c4 = zyaw()
                if abs(float(s["ref_yaw"]) - ysum) < par.yaw_tol:
                    s["completed_turn"] = 1
        else:
            s["status"] = 5
            c3, c4 = zyaw()
        if t is not None:
            t["ticks"][int(s["status"])] += 1
            t["failed"] += int(failed)
            if s["completed_mission"] and t["first_done"] < 0:
                t["first_done"] = k
            if s["status"] == 0:
                e = rng - par.safety_dis
                t["standoff_sq"] = float(t["standoff_sq"]) + e * e
    rec = np.zeros((), dtype=RESULT_DTYPE)
    rec["u0"] = [c1, c2, -c3, c4]
    rc = ROTOR_CONSTANT
    rec["thrust"] = [((-c1 + c2) + c4) / rc, ((-c1 - c2) - c4) / rc, ((c1 + c2) - c4) / rc, ((c1 - c2) + c4) / rc, c3 / rc, c3 / rc]
    return rec, failed


def control_batch(par, state, stats, rng, z, psi):
    """the batch: (state_out, records, stats_out or None, failed [B]); the inputs are left as they are"""
    so = state.copy()
    to = None if stats is None else stats.copy()
    rec, failed = np.zeros(len(so), dtype=RESULT_DTYPE), np.zeros(len(so), dtype=bool)
    for b in range(len(so)):
        rec[b], failed[b] = control(par, so[b], None if to is None else to[b], rng[b], z[b], psi[b])
    return so, rec, to, failed


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
