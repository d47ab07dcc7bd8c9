#!/usr/bin/env python3
"""Writes tests/golden/eskf_exact.npz: inputs of the error-state filter's ticks, the 60-digit results (tests/eskf_exact.py) rounded to double, and per
regime, family and quantity the worst error E_np of the numpy restatement against that reference -- the bar of tests/test_gpu_eskf_exact.py.
Needs mpmath; no GPU, no library.  Deterministic (seeded).

Regimes: shipped (the defaults), varied (pairwise different Q and R12 entries, vel_inject = 1, inject_bias_g = 1), loop (dt = gps_dt = 0.05,
compensate_coef = rotor_constant = 1).  Families: nominal, tiny_angles (attitude innovation and w dt below 1e-9: the series of exp and log),
large_angle (attitude innovation near 3 rad; one case with w < 0 in q^-1 * q_meas), zero_motion, predict_only, prediction_left
(P = -(A A' + I / 2): the first pivot of S is negative, status 1), chain (3 filters x 6 ticks, predict-only and update ticks alternating).
What a family claims is asserted here on the reference itself: status, the sign of every pivot, the size of the angles."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eskf_exact as X  # noqa: E402

REGIMES = ("shipped", "varied", "loop")
FAMILIES = ("nominal", "tiny_angles", "large_angle", "zero_motion", "predict_only", "prediction_left", "chain")
COUNT = {"nominal": 8, "tiny_angles": 2, "large_angle": 3, "zero_motion": 2, "predict_only": 3, "prediction_left": 2}
CHAIN_B, CHAIN_K = 3, 6
NPOOL = 6


def regime_vector(name):
    v = X.default_par_vector()
    d = {f: (sum(n for _, n in X.PAR_FIELDS[:k]), n) for k, (f, n) in enumerate(X.PAR_FIELDS)}

    def put(f, val):
        o, n = d[f]
        v[o:o + n] = val
    if name == "varied":
        put("Q", 0.001 * (1.0 + 0.37 * np.arange(21)))
        put("R12", np.array([0.01, 0.013, 0.008, 0.02, 0.017, 0.024, 0.0006, 0.0009, 0.0005, 0.012, 0.015, 0.011]))
        put("vel_inject", 1.0)
        put("inject_bias_g", 1.0)
    elif name == "loop":
        put("dt", 0.05); put("gps_dt", 0.05); put("compensate_coef", 1.0); put("rotor_constant", 1.0)
    return v


def quat_from_rotvec(phi):
    return X.np_unit(X.np_exp(np.asarray(phi, dtype=np.float64)))


def draw_state(rng):
    x = np.zeros(X.NX)
    x[0:3] = rng.uniform(-5, 5, 3) + np.array([0, 0, -20.0])
    x[3:6] = rng.normal(size=3) * 0.5
    x[6:10] = X.np_unit(X.np_qmul(quat_from_rotvec([0, 0, rng.uniform(-3, 3)]), quat_from_rotvec(rng.uniform(-0.5, 0.5, 3) * np.array([1, 1, 0]))))
    x[10:13] = rng.normal(size=3) * 1e-3
    x[13:16] = rng.normal(size=3) * 1e-2
    x[16:19] = np.array([0, 0, -9.81]) + rng.normal(size=3) * 0.01
    x[19:22] = rng.uniform(-5, 5, 3)
    return x


def draw_pool(rng):
    pool = []
    for k in range(NPOOL):
        A = rng.normal(size=(X.NE, X.NE)) * 0.1
        P = A @ A.T + np.diag(rng.uniform(0.01, 0.1, X.NE))
        pool.append(X.from_triu(X.to_triu(P)))      # exactly symmetric
    return np.array(pool)


def consistent_inputs(rng, p, x, P, angle=None, flip=False):
    """imu, gps_p, gps_v, q_meas, thrust around the prediction of x; angle: the size of the attitude innovation (None: 0.02 rad noise)"""
    R = X.np_rot(X.np_unit(x[6:10]))
    imu = np.concatenate([R.T @ (rng.normal(size=3) * 0.3 - x[16:19]) + x[13:16], rng.normal(size=3) * 0.3 + x[10:13]])
    pred = X.np_tick(p, x, P, imu, update=False)["x_pred"]
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    phi = rng.normal(size=3) * 0.02 if angle is None else axis * angle
    qm = X.np_unit(X.np_qmul(pred[6:10], X.np_exp(phi)))
    if flip:
        qm = -qm
    return imu, pred[0:3] + rng.normal(size=3) * 0.05, pred[3:6] + rng.normal(size=3) * 0.05, qm, rng.uniform(-4, 4, 6)


def main():
    rng = np.random.default_rng(20261021)
    pool = draw_pool(rng)
    out = {k: [] for k in ("regime", "family", "input", "x0", "imu", "gps_p", "gps_v", "qm", "thrust", "xn", "Pnu", "xi", "xw", "mp", "status", "pivots")}
    neg_pool = []
    for k in range(2):
        A = rng.normal(size=(X.NE, X.NE)) * 0.1
        neg_pool.append(X.from_triu(X.to_triu(-(A @ A.T + np.eye(X.NE) / 2))))
    P_all = np.concatenate([pool, np.array(neg_pool)])
    E_np = np.full((len(REGIMES), len(FAMILIES), 4), np.nan)
    chain = {k: [] for k in ("x0", "input", "imu", "gps_p", "gps_v", "qm", "thrust", "xn", "Pnu", "xw", "mp", "update")}
    for ri, rname in enumerate(REGIMES):
        vec = regime_vector(rname)
        p, ex = X.par_dict(vec), X.ExactEskf(vec)
        for fi, fam in enumerate(FAMILIES[:-1]):
            worst = np.zeros(4)
            for k in range(COUNT[fam]):
                pi = NPOOL + k if fam == "prediction_left" else (k if fam == "zero_motion" else int(rng.integers(NPOOL)))
                P = P_all[pi]
                x = draw_state(rng)
                upd = fam != "predict_only"
                if fam == "zero_motion":
                    x = np.zeros(X.NX); x[6] = 1.0; x[18] = -p["g"]
                    imu, gp, gv, qm, th = np.array([0, 0, p["g"], 0, 0, 0.0]), np.zeros(3), np.zeros(3), np.array([1.0, 0, 0, 0]), np.zeros(6)
                elif fam == "tiny_angles":
                    imu, gp, gv, qm, th = consistent_inputs(rng, p, x, P, angle=0.0)
                    imu[3:6] = x[10:13] + rng.normal(size=3) * 1e-9      # w dt ~ 1e-10
                    pred = X.np_tick(p, x, P, imu, update=False)["x_pred"]
                    qm = X.np_unit(X.np_qmul(pred[6:10], X.np_exp(rng.normal(size=3) * 2e-10)))
                elif fam == "large_angle":
                    imu, gp, gv, qm, th = consistent_inputs(rng, p, x, P, angle=3.0 - 0.02 * k, flip=(k == 1))
                else:
                    imu, gp, gv, qm, th = consistent_inputs(rng, p, x, P)
                ref = ex.tick_double(x, P, imu, gp, gv, qm, th, update=upd)
                dbl = X.np_tick(p, x, P, imu, gp, gv, qm, th, update=upd)
                # ---- what the family claims, on the reference itself
                piv = ref["pivots"]
                if fam == "prediction_left":
                    assert ref["status"] == 1 and piv[0] < 0 and np.isnan(piv[1:]).all(), (rname, fam, piv)
                    assert dbl["status"] == 1
                elif upd:
                    assert ref["status"] == 0 and (piv > 0).all(), (rname, fam, piv)
                    assert dbl["status"] == 0
                else:
                    assert ref["status"] == 0 and np.isnan(piv).all()
                if fam == "tiny_angles":
                    assert 0 < ref["angle_pred"] < 1e-9 and 0 < ref["angle_innov"] < 1e-9, (ref["angle_pred"], ref["angle_innov"])
                if fam == "large_angle":
                    assert 2.9 < ref["angle_innov"] < 3.05, ref["angle_innov"]
                    qp = ref["x_pred"][6:10]
                    wprod = X.np_qmul(np.array([qp[0], -qp[1], -qp[2], -qp[3]]), X.np_unit(qm))[0]
                    assert (wprod < 0) == (k == 1), (k, wprod)
                if fam == "zero_motion":
                    assert np.abs(ref["x_pred"][0:6]).max() == 0.0 and np.array_equal(ref["x_pred"][6:10], [1, 0, 0, 0])
                e = X.errors((dbl["x_new"][None], dbl["P_new"][None], dbl["xi_world"][None], dbl["mpc_p"][None]),
                             (ref["x_new"][None], ref["P_new"][None], ref["xi_world"][None], ref["mpc_p"][None]))[:, 0]
                worst = np.maximum(worst, e)
                for key, val in (("regime", ri), ("family", fi), ("input", pi), ("x0", x), ("imu", imu), ("gps_p", gp), ("gps_v", gv), ("qm", qm),
                                 ("thrust", th), ("xn", ref["x_new"]), ("Pnu", X.to_triu(ref["P_new"])), ("xi", ref["xi"]), ("xw", ref["xi_world"]),
                                 ("mp", ref["mpc_p"]), ("status", ref["status"]), ("pivots", piv)):
                    out[key].append(val)
            E_np[ri, fi] = worst
            print(rname, fam, " ".join(f"{v:.2e}" for v in worst), flush=True)
        # ---- the chain: the reference carries its state at 60 digits, the restatement its own in double
        fi = FAMILIES.index("chain")
        worst = np.zeros(4)
        cx0 = np.array([draw_state(rng) for _ in range(CHAIN_B)])
        cin = rng.integers(NPOOL, size=CHAIN_B)
        rec = {k: np.zeros((CHAIN_K, CHAIN_B) + s) for k, s in (("imu", (6,)), ("gps_p", (3,)), ("gps_v", (3,)), ("qm", (4,)), ("thrust", (6,)),
                                                                 ("xn", (X.NX,)), ("Pnu", (len(X.IU[0]),)), ("xw", (3,)), ("mp", (4,)))}
        for b in range(CHAIN_B):
            xm, Pm = list(cx0[b]), [list(r) for r in pool[cin[b]]]
            xd, Pd = cx0[b].copy(), pool[cin[b]].copy()
            for k in range(CHAIN_K):
                upd = k % 2 == 1
                imu, gp, gv, qm, th = consistent_inputs(rng, p, xd, Pd)
                r = ex.tick(xm, Pm, imu, gp, gv, qm, th, update=upd)
                xm, Pm = r["x_new"], r["P_new"]
                ref = ex.rounded(r)
                assert ref["status"] == 0 and (not upd or (ref["pivots"] > 0).all())
                dbl = X.np_tick(p, xd, Pd, imu, gp, gv, qm, th, update=upd)
                xd, Pd = dbl["x_new"], dbl["P_new"]
                e = X.errors((dbl["x_new"][None], dbl["P_new"][None], dbl["xi_world"][None], dbl["mpc_p"][None]),
                             (ref["x_new"][None], ref["P_new"][None], ref["xi_world"][None], ref["mpc_p"][None]))[:, 0]
                worst = np.maximum(worst, e)
                for key, val in (("imu", imu), ("gps_p", gp), ("gps_v", gv), ("qm", qm), ("thrust", th), ("xn", ref["x_new"]),
                                 ("Pnu", X.to_triu(ref["P_new"])), ("xw", ref["xi_world"]), ("mp", ref["mpc_p"])):
                    rec[key][k, b] = val
        E_np[ri, fi] = worst
        print(rname, "chain", " ".join(f"{v:.2e}" for v in worst), flush=True)
        chain["x0"].append(cx0); chain["input"].append(cin)
        chain["update"].append(np.arange(CHAIN_K) % 2 == 1)
        for key in rec:
            chain[key].append(rec[key])
    data = {k: np.array(v) for k, v in out.items()}
    data.update({"chain_" + k: np.array(v) for k, v in chain.items()})
    data.update(regimes=np.array(REGIMES), families=np.array(FAMILIES), quantities=np.array(X.QUANTITIES),
                par=np.array([regime_vector(r) for r in REGIMES]), P0u=X.to_triu(P_all), E_np=E_np, digits=np.array(X.DIGITS))
    path = os.path.join(ROOT, "tests", "golden", "eskf_exact.npz")
    np.savez(path, **data)
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(ROOT, "tests", "golden", "ekf_exact.npz"))
    assert size <= limit, (size, limit)
    print(f"wrote {path}: {size} bytes, {len(data['regime'])} single ticks, {len(REGIMES)} chains")


if __name__ == "__main__":
    main()
