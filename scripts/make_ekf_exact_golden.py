#!/usr/bin/env python3
"""Build tests/golden/ekf_exact.npz: single ticks and short chains of the EKF disturbance observer at the states where the structured
kernel can be wrong unnoticed, in parameter regimes where two correct FP64 evaluations agree to 1e-13, with the results of the same
filter at 60 digits (tests/ekf_exact.py, rounded to double) and the errors of the two double implementations -- the C oracle and the
numpy restatement test_oracle_ekf.np_update -- against them.  Fixed seeds, no input but this file: running it again gives the same
bytes, with the same C compiler, libm and numpy (E_orc and E_np are what the locally built oracle and numpy give; inputs and exact
results do not depend on them).

    python scripts/make_ekf_exact_golden.py [--check]        (--check: compare with the committed file instead of writing it)

Regimes (a brov_ekf_params each, `par` [regimes][84] in the field order of the structure):
    shipped      the defaults (fd_step 1e-6, R = dt^4 / 4, Q of two distinct values)
    tight        fd_step 2^-7, R 1, Q of 18 pairwise different entries over the default's range
    mid          fd_step 2^-10, R 1e-2, the same Q
    device_loop  tight, with K's rows 2, 3 zeroed and compensate_coef = rotor_constant = 1 (tests/test_gpu_ekf.test_device_loop_with_solver)
    varied       tight, with dt, mass, added_mass, Dl, Dnl varied: the zero pattern is the model's, not its numbers'
Families: nominal; zero_motion (angles, velocities, rates exactly 0: the forward difference steps across the kink of |v| v); zero_dist
(disturbances exactly 0); far_yaw (yaw of several hundred rad, roll and pitch up to +-1); cov_scaled (covariances scaled by 1e-6 .. 10);
prediction_only (P = -(A A' + I / 2): the first pivot of S is negative, the result is the prediction -- F, G = P F', F G + Q and the
symmetric fill apart from the gain and the Joseph form); chain (3 filters x 6 ticks, tight and shipped: the reference carries its state
at 60 digits, the double implementations theirs in double).

The estimates and covariances a tick starts from (x0, P0u: the upper triangle) are shared by the regimes -- a regime uses the first
COUNT[regime] of every family -- and thrust, y12, acc are drawn per regime, consistent with its constants.  That, upper triangles and
the case counts keep the file below the largest fixture committed so far; the price is 6 cases per family in shipped and tight, 3 in mid and
varied and 2 in device_loop.

Arrays: regimes, families, quantities (names); par; x0 [m,18], P0u [m,171], in_family [m]; per case (n, in regime and family order):
regime, family, input (row of x0 / P0u), thrust, y12, acc, piv_first, piv_min (pivots of S without row exchanges; piv_min over those met),
status, xn [n,18], Pnu [n,171], wf [n,6], mp [n,4], fd_bound [n,4] (ekf_exact.fd_rounding_bound: what the rounding of the forward differences
can do to first order, scaled like the errors; zero for prediction_only); pred_case [k], pred_x, pred_Pu: the prediction of the first nominal case of every
regime (what a tick with a NaN acceleration must leave); chain_regime [2], chain_x0 [3,18], chain_P0u [3,171], chain_thrust / _y12 / _acc
[2,6,3,.], chain_xn / _Pnu / _wf / _mp [2,6,3,.], chain_piv_min [2,6,3]; E_orc, E_np [regimes, families, quantities]: the worst scaled
error of the C oracle / of np_update on the family (x, wf, mpc_p: |got - ref| / max(1, |ref|); P: |got - ref| / max |ref| per filter),
NaN where a regime has no such family.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "tests", "golden", "ekf_exact.npz")

REGIMES = ("shipped", "tight", "mid", "device_loop", "varied")
FAMILIES = ("nominal", "zero_motion", "zero_dist", "far_yaw", "cov_scaled", "prediction_only", "chain")
SINGLE = FAMILIES[:6]
COUNT = dict(shipped=6, tight=6, mid=3, device_loop=2, varied=3)
N_INPUTS = 6
COV_EXPONENTS = (-6, 1, -3, -1, -4, 0)      # the two ends first: every regime has them
CHAIN_REGIMES, CHAIN_FILTERS, CHAIN_TICKS = ("tight", "shipped"), 3, 6
CHAIN_BOUND = 2.0      # |x_new - truth| of the reference, every entry and tick (the estimate starts up to ~1.5 beside the truth)


def regime_params(default):
    """regime -> parameter vector; `default`: the defaults' (ekf_exact.par_vector)"""
    from ekf_exact import par_dict, PAR_FIELDS
    off, o = {}, 0
    for f, n in PAR_FIELDS:
        off[f] = slice(o, o + n); o += n
    d = par_dict(default)
    q = np.geomspace(d["Q"].min(), d["Q"].max(), 18)[np.random.default_rng(1805).permutation(18)]
    assert len(set(q)) == 18
    out = {"shipped": default.copy()}
    for name, step, R in (("tight", 2.0 ** -7, 1.0), ("mid", 2.0 ** -10, 1e-2), ("device_loop", 2.0 ** -7, 1.0), ("varied", 2.0 ** -7, 1.0)):
        v = default.copy()
        v[off["fd_step"]], v[off["R"]], v[off["Q"]] = step, R, q
        out[name] = v
    v = out["device_loop"]
    v[off["K"]][12:24] = 0.0
    v[off["compensate_coef"]] = v[off["rotor_constant"]] = 1.0
    v = out["varied"]
    v[off["dt"]] *= 0.6; v[off["mass"]] *= 1.3
    v[off["added_mass"]] *= np.array([1.2, 1.0, 0.8, 1.0, 1.5, 0.7])
    v[off["Dl"]] *= np.array([0.8, 1.1, 0.9, 1.2, 0.7, 1.3])
    v[off["Dnl"]] *= np.array([1.25, 0.8, 1.1, 0.6, 1.4, 0.9])
    return out


def shared_inputs():
    """x0 [m,18], P0 [m,18,18], family [m]: the estimates and covariances of the single ticks"""
    import test_oracle_ekf as T
    xs, Ps, fam = [], [], []
    for fi, name in enumerate(SINGLE):
        rng = np.random.default_rng(4100 + fi)
        for i in range(N_INPUTS):
            x = T.rand_state(rng); x[15:17] *= 0.05
            A = rng.normal(size=(18, 18)) * 0.3
            P = A @ A.T + np.eye(18) * 0.5
            if name == "zero_motion":
                x[3:12] = 0.0
            elif name == "zero_dist":
                x[12:18] = 0.0
            elif name == "far_yaw":
                x[5] = (1 if i % 2 else -1) * rng.uniform(200.0, 400.0); x[3:5] = rng.uniform(-1.0, 1.0, 2)
                if i < 2:
                    x[3 + i] = (1.0, -1.0)[i]
            elif name == "cov_scaled":
                P = P * 10.0 ** COV_EXPONENTS[i]
            elif name == "prediction_only":
                P = -P
            xs.append(x); Ps.append(0.5 * (P + P.T)); fam.append(fi)
    return np.array(xs), np.array(Ps), np.array(fam, dtype=np.int32)


def build(progress=False):
    from ekf_exact import Doubles, ExactEkf, errors, fd_rounding_bound, par_vector, to_triu, QUANTITIES
    import test_oracle_ekf as T
    from oracle.oracle_ffi import EkfOracle, build as build_oracle
    build_oracle()
    par = regime_params(par_vector(EkfOracle().par))
    x0, P0, in_family = shared_inputs()
    nq = len(QUANTITIES)
    E_orc = np.full((len(REGIMES), len(FAMILIES), nq), np.nan); E_np = E_orc.copy()
    rows = {k: [] for k in ("regime", "family", "input", "thrust", "y12", "acc", "piv_first", "piv_min", "status", "xn", "Pnu", "wf", "mp", "fd_bound")}
    pred = {k: [] for k in ("pred_case", "pred_x", "pred_Pu")}
    for ri, rname in enumerate(REGIMES):
        D, X = Doubles(par[rname]), ExactEkf(par[rname])
        for fi, fname in enumerate(SINGLE):
            rng = np.random.default_rng(5200 + 16 * ri + fi)
            eo, en = [], []
            for i in range(COUNT[rname]):
                m = fi * N_INPUTS + i
                assert in_family[m] == fi
                x, P = x0[m], P0[m]
                thrust, y12, acc = D.consistent_inputs(rng, x)
                r = X.tick_double(x, P, thrust, y12, acc)
                only = fname == "prediction_only"
                if only:
                    assert r["status"] == 1 and r["pivots"][0] < 0 and np.isnan(r["pivots"][1:]).all(), (rname, i, r["pivots"])
                else:
                    assert r["status"] == 0 and np.all(r["pivots"] > 0), (rname, fname, i, r["pivots"])
                ref = (r["x_new"], r["P_new"], r["wf"], r["mpc_p"])
                eo.append(errors(D.oracle(x, P, thrust, y12, acc, prediction=only), ref))
                en.append(errors(D.numpy(x, P, thrust, y12, acc, prediction=only), ref))
                if fi == 0 and i == 0:
                    pred["pred_case"].append(len(rows["regime"])); pred["pred_x"].append(r["x_pred"]); pred["pred_Pu"].append(to_triu(r["P_pred"]))
                for k, v in (("regime", ri), ("family", fi), ("input", m), ("thrust", thrust), ("y12", y12), ("acc", acc),
                             ("piv_first", r["pivots"][0]), ("piv_min", np.nanmin(r["pivots"])), ("status", r["status"]),
                             ("xn", r["x_new"]), ("Pnu", to_triu(r["P_new"])), ("wf", r["wf"]), ("mp", r["mpc_p"]),
                             ("fd_bound", np.zeros(4) if only else fd_rounding_bound(D, x, P, thrust, y12, acc))):
                    rows[k].append(v)
            E_orc[ri, fi], E_np[ri, fi] = np.max(eo, axis=0), np.max(en, axis=0)
            if progress:
                print(f"{rname:12s} {fname:16s} n = {COUNT[rname]}   E_orc " + " ".join(f"{v:.1e}" for v in E_orc[ri, fi]) +
                      "   E_np " + " ".join(f"{v:.1e}" for v in E_np[ri, fi]), flush=True)
    # ---- chains: one truth per filter, driven by the regime's own model; the estimate starts beside it.  The filter's one-step map is
    # unstable in the roll rate (Dl[3] dt / Ix = -4.2, beyond what an RK4 step damps) and only the update holds it: a draw on which the
    # REFERENCE leaves its truth by more than CHAIN_BOUND within the six ticks, in either regime, is drawn again -- judged on the reference alone
    B, K = CHAIN_FILTERS, CHAIN_TICKS
    DX = {r: (Doubles(par[r]), ExactEkf(par[r])) for r in CHAIN_REGIMES}

    def chain_draw(cand):
        rng = np.random.default_rng(6300 + cand)
        truth = T.rand_state(rng); truth[15:17] *= 0.05
        x = truth + np.concatenate([rng.normal(size=12) * 0.02, rng.normal(size=6) * 0.5 * np.array([1, 1, 1, 0.05, 0.05, 1])])
        A = rng.normal(size=(18, 18)) * 0.3
        P = A @ A.T + np.eye(18) * 0.5
        return truth, x, 0.5 * (P + P.T), rng.uniform(-4, 4, (K, 6)), rng.normal(size=(K, 12)) * 1e-3, rng.normal(size=(K, 6)) * 0.01

    def chain_run(rname, draw):
        """the six ticks of one filter: None if the reference fails or strays, else (inputs and rounded results per tick, oracle's and numpy's errors)"""
        truth, x, P, thrusts, ny, na = draw
        D, X = DX[rname]
        c = D.c
        xt, xe, Pe = truth.copy(), x, P                                  # the reference's state: doubles at first, then 60 digits
        xo, Po, xn, Pn = x.copy(), P.copy(), x.copy(), P.copy()
        ticks, eo, en = [], [], []
        for k in range(K):
            thrust = thrusts[k]
            tau = c["K"] @ thrust
            h = c["dt"] / 10                                             # the truth: ten classical RK4 steps
            for _ in range(10):
                k1 = T.np_f(c, xt, tau); k2 = T.np_f(c, xt + h / 2 * k1, tau); k3 = T.np_f(c, xt + h / 2 * k2, tau); k4 = T.np_f(c, xt + h * k3, tau)
                xt = xt + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
            y12 = xt[:12] + ny[k]
            acc = T.np_f(c, xt, tau)[6:12] + na[k]                       # at the END of the step: h is evaluated at x_pred
            out = X.tick(xe, Pe, thrust, y12, acc)
            r = X.rounded(out)
            if out["status"] != 0 or not np.abs(r["x_new"] - xt).max() <= CHAIN_BOUND:
                return None
            xe, Pe = out["x_new"], out["P_new"]
            ref = (r["x_new"], r["P_new"], r["wf"], r["mpc_p"])
            o = D.oracle(xo, Po, thrust, y12, acc); xo, Po = o[0], o[1]
            n = D.numpy(xn, Pn, thrust, y12, acc); xn, Pn = n[0], n[1]
            eo.append(errors(o, ref)); en.append(errors(n, ref))
            ticks.append((thrust, y12, acc, r))
        return ticks, eo, en

    kept, cand = [], 0
    while len(kept) < B:
        draw = chain_draw(cand)
        runs = [chain_run(r, draw) for r in CHAIN_REGIMES]
        if all(v is not None for v in runs):
            kept.append((draw, runs))
        elif progress:
            print(f"chain draw {cand}: the reference strays in {[r for r, v in zip(CHAIN_REGIMES, runs) if v is None]}, drawn again", flush=True)
        cand += 1
        assert cand < 20
    cx0, cP0 = np.stack([d[1] for d, _ in kept]), np.stack([d[2] for d, _ in kept])
    ch = dict(chain_thrust=np.empty((2, K, B, 6)), chain_y12=np.empty((2, K, B, 12)), chain_acc=np.empty((2, K, B, 6)),
              chain_xn=np.empty((2, K, B, 18)), chain_Pnu=np.empty((2, K, B, 171)), chain_wf=np.empty((2, K, B, 6)), chain_mp=np.empty((2, K, B, 4)),
              chain_piv_min=np.empty((2, K, B)))
    fi = FAMILIES.index("chain")
    for ci, rname in enumerate(CHAIN_REGIMES):
        ri = REGIMES.index(rname)
        eo, en = [], []
        for b, (_, runs) in enumerate(kept):
            ticks, e1, e2 = runs[ci]
            eo += e1; en += e2
            for k, (thrust, y12, acc, r) in enumerate(ticks):
                ch["chain_thrust"][ci, k, b], ch["chain_y12"][ci, k, b], ch["chain_acc"][ci, k, b] = thrust, y12, acc
                ch["chain_xn"][ci, k, b], ch["chain_Pnu"][ci, k, b] = r["x_new"], to_triu(r["P_new"])
                ch["chain_wf"][ci, k, b], ch["chain_mp"][ci, k, b], ch["chain_piv_min"][ci, k, b] = r["wf"], r["mpc_p"], np.min(r["pivots"])
        E_orc[ri, fi], E_np[ri, fi] = np.max(eo, axis=0), np.max(en, axis=0)
        if progress:
            print(f"{rname:12s} {'chain':16s} n = {B} x {K}   E_orc " + " ".join(f"{v:.1e}" for v in E_orc[ri, fi]) +
                  "   E_np " + " ".join(f"{v:.1e}" for v in E_np[ri, fi]), flush=True)
    out = dict(regimes=np.array(REGIMES), families=np.array(FAMILIES), quantities=np.array(QUANTITIES),
               par=np.stack([par[r] for r in REGIMES]), x0=x0, P0u=to_triu(P0), in_family=in_family)
    for k, v in rows.items():
        out[k] = np.array(v, dtype=np.int32) if k in ("regime", "family", "input", "status") else np.array(v, dtype=np.float64)
    out["pred_case"] = np.array(pred["pred_case"], dtype=np.int32)
    out["pred_x"], out["pred_Pu"] = np.array(pred["pred_x"]), np.array(pred["pred_Pu"])
    out["chain_regime"] = np.array([REGIMES.index(r) for r in CHAIN_REGIMES], dtype=np.int32)
    out["chain_x0"], out["chain_P0u"] = cx0, to_triu(cP0)
    out.update(ch)
    out["E_orc"], out["E_np"] = E_orc, E_np
    return out


def main():
    from make_model_exact_golden import save_npz      # the writer with fixed member times
    out = build(progress=True)
    if "--check" in sys.argv:
        tmp = OUT + ".check"
        save_npz(tmp, out)
        same = open(tmp, "rb").read() == open(OUT, "rb").read()
        os.remove(tmp)
        print("identical to the committed fixture" if same else "DIFFERS from the committed fixture")
        sys.exit(0 if same else 1)
    save_npz(OUT, out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(out['regime'])} single ticks, {2 * CHAIN_FILTERS * CHAIN_TICKS} chained")


if __name__ == "__main__":
    main()
