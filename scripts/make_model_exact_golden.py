#!/usr/bin/env python3
"""Build tests/golden/model_exact.npz: inputs of the device model at the places where a kernel can be wrong unnoticed, with the exact
f, x+ and S = d x+ / d [x; u] of tests/model_exact.py (60 digits, rounded to double) and the double-precision oracle's own error against
them.  Fixed seeds, no input but this file: running it again gives the same bytes -- with the same C compiler and libm, since e_orc and
E_orc are what the locally built oracle (oracle/bluerov2_oracle.c, libm's sin and cos) gives; inputs and exact results do not depend on them.

    python scripts/make_model_exact_golden.py [--check]        (--check: compare with the committed file instead of writing it)

Arrays (n cases, in family order):
    family [n] index into `families`;  h [n];  x [n,12], u [n,4], p [n,16];  ww [n,6] world-frame wrench, rp [n,2] roll / pitch moments
    (zero where the family has none);  f [n,12], xn [n,12], S [n,12,16] exact, rounded to double (S is zero for the world-wrench family:
    no kernel linearises under one);  e_orc [n,3]: the oracle's worst scaled error |got - ref| / max(1, |ref|) of the case for f, x+, S;
    E_orc [families,3]: its maximum per family (NaN: S of the world-wrench family).
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "model_exact.npz")

FAMILIES = ("wide", "quadrant_edges", "kinks", "far_yaw", "steep_pitch", "parameters", "world_wrench", "dist6")
COUNT = dict(wide=24, quadrant_edges=48, kinks=24, far_yaw=16, steep_pitch=16, parameters=16, world_wrench=24, dist6=16)
STEPS = (0.0125, 0.05, 0.1)
P_NOMINAL = np.array([0, 0, 0, 0, 1.7182, 0, 5.468, 0.4006, -11.7391, -20, -31.8678, -5, -18.18, -21.66, -36.99, -1.55])
U_BOX = 50.0     # the default input box
S_MAX = 50.0     # a case is kept if no entry of d x+ / d [x; u] exceeds this (nominal steps: ~10; an unstable step: 1e3 and up)


def wide_case(rng, i):
    """the common draw: phi in [-pi, pi], |theta| <= 1.3, |psi| <= 400, |v| <= 2 m/s, rates <= 1 rad/s, disturbances <= 300, the other
    parameters +-30 %, inputs +-20 with every fourth draw holding one or two inputs at a bound (cases() halves the inputs of a draw whose
    step is badly conditioned, so fewer cases keep one there: tests/test_model_exact_cpu.py asserts that every family still has some)"""
    x = np.empty(12)
    x[:3] = rng.uniform(-20, 20, 3)
    x[3], x[4], x[5] = rng.uniform(-np.pi, np.pi), rng.uniform(-1.3, 1.3), rng.uniform(-400, 400)
    x[6:9] = rng.uniform(-2, 2, 3)
    x[9:12] = rng.uniform(-1, 1, 3)
    u = rng.uniform(-20, 20, 4)
    if i % 4 == 3:
        u[i % 3] = U_BOX * (1 if i % 8 == 3 else -1)     # on the bound (kept where the step stays well conditioned: see S_MAX)
        if i % 8 == 7:
            u[3] = U_BOX
    p = P_NOMINAL.copy()
    p[:4] = rng.uniform(-300, 300, 4)
    p[4:] *= rng.uniform(0.7, 1.3, 12)
    return x, u, p


def near(mp, k, half, nb):
    """the double nearest to k pi/2 (half: (k + 1/2) pi/2), moved nb doubles up (nb = -1, 0, 1)"""
    v = float(mp.pi * (mp.mpf(2 * k + 1) / 4 if half else mp.mpf(k) / 2))
    if nb:
        v = float(np.nextafter(v, np.inf if nb > 0 else -np.inf))
    return v


def cases(mp, well_conditioned):
    """yields (family, x, u, p, h, ww, rp).  A draw whose step is badly conditioned (well_conditioned(...) false: thrust of tens of newtons
    on a vehicle of a few kilograms over 0.1 s outruns what one ERK4 step integrates stably) is tried at the next smaller step, then drawn
    again with the inputs halved: the families probe the model's corners, not the integrator's stability limit."""
    for fi, fam in enumerate(FAMILIES):
        rng = np.random.default_rng(20240 + fi)
        for i in range(COUNT[fam]):
            for attempt in range(8):
                x, u, p, h, ww, rp = one_case(mp, fam, rng, i)
                u = u * 0.5 ** attempt
                hs = [s for s in STEPS if s <= h][::-1]
                h = next((s for s in hs if well_conditioned(x, u, p, s, ww, rp)), None)
                if h is not None:
                    break
            else:
                raise RuntimeError(f"no well-conditioned draw for {fam} case {i}")
            yield fi, x, u, p, h, ww, rp


def one_case(mp, fam, rng, i):
    z6, z2 = np.zeros(6), np.zeros(2)
    x, u, p = wide_case(rng, i)
    h, ww, rp = STEPS[i % 3], z6, z2
    if fam == "quadrant_edges":
        half, j = i % 2, i // 6
        k_psi = (1, -2, 3, -4, -253, 254, -251, 252)[j]           # every residue mod 4 with both signs, up to |psi| ~ 400
        k_phi = ((0, 1, -1, 2, -2, 1, -1, 0), (0, -1, 1, -2, 0, -1, 1, -2))[half][j]
        x[5] = near(mp, k_psi, half, (i // 2) % 3 - 1)
        x[3] = near(mp, k_phi, half, (i // 2 + 1) % 3 - 1)
        x[4] = near(mp, (0, -1)[j % 2] if half else 0, half, (i // 2 + 2) % 3 - 1)    # 0 or +-pi/4: away from +-pi/2
    elif fam == "kinks":
        vel = (6, 7, 8, 11)
        if i < 16:
            special = (0.0, -0.0, 1e-300, -1e-300)
            mask = i % 15 + 1                                       # which of u, v, w, r sit on the kink
            for b, c in enumerate(vel):
                if mask >> b & 1:
                    x[c] = special[(i + b) % 4]
        else:
            # a velocity of a few 1e-3 that changes sign inside the step: the input pushes against it
            s = 1.0 if i % 2 else -1.0
            p[:4] = rng.uniform(-3, 3, 4)
            u[:] = rng.uniform(-1, 1, 4)
            which = i % 3
            if which == 0:
                x[6], u[0] = 3e-3 * s, 5.0 * s
            elif which == 1:
                x[8], u[2] = 2e-3 * s, 5.0 * s
            else:
                x[11], u[3] = 4e-3 * s, -5.0 * s
            if i >= 21:
                x[7] = 0.0
    elif fam == "far_yaw":
        x[5] = (1 if i % 2 else -1) * 10.0 ** rng.uniform(np.log10(400.0), 5.0)
    elif fam == "steep_pitch":
        x[4] = (1 if i % 2 else -1) * rng.uniform(1.3, 1.5)
    elif fam == "parameters":
        p[4:7] = 10.0 ** rng.uniform(0.0, np.log10(50.0), 3) - 11.26     # m + added mass from 1 to 50
        if i == 0:
            p[4:7] = np.array([1.0, 50.0, 1.0]) - 11.26
        p[7] = 10.0 ** rng.uniform(np.log10(0.3), np.log10(3.0)) - 0.58  # Iz + added inertia from 0.3 to 3
        if i % 3 == 0:
            p[8:12] = 0.0
        elif i % 3 == 1:
            p[12:16] = 0.0
    elif fam == "world_wrench":
        ww = np.concatenate([rng.uniform(-300, 300, 3), rng.uniform(-50, 50, 3)])
    elif fam == "dist6":
        rp = rng.uniform(-5, 5, 2)
    return x, u, p, h, ww, rp


def save_npz(path, arrays):
    """numpy.savez_compressed with fixed member times: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def build():
    from model_exact import ExactModel, MpBackend, scaled_err
    from wrench_restatement import f_under_wrench, rk4_under_wrench
    from oracle.oracle_ffi import Oracle, build as build_oracle
    build_oracle()
    orc = Oracle()
    M = ExactModel(MpBackend())
    cache = {}

    def well_conditioned(x, u, p, h, ww, rp):
        xn, S = M.sens(x, u, p, h, ww if ww.any() else None, rp if rp.any() else None)
        cache[(x.tobytes(), u.tobytes(), p.tobytes(), h)] = (xn, S)
        return np.abs(S).max() <= S_MAX

    cs = list(cases(M.K.mp, well_conditioned))
    n = len(cs)
    out = dict(family=np.empty(n, dtype=np.int32), h=np.empty(n), x=np.empty((n, 12)), u=np.empty((n, 4)), p=np.empty((n, 16)),
               ww=np.zeros((n, 6)), rp=np.zeros((n, 2)), f=np.empty((n, 12)), xn=np.empty((n, 12)), S=np.zeros((n, 12, 16)),
               e_orc=np.full((n, 3), np.nan))
    wf, d6 = FAMILIES.index("world_wrench"), FAMILIES.index("dist6")
    for c, (fi, x, u, p, h, ww, rp) in enumerate(cs):
        out["family"][c], out["h"][c], out["x"][c], out["u"][c], out["p"][c], out["ww"][c], out["rp"][c] = fi, h, x, u, p, ww, rp
        a_ww, a_rp = (ww if fi == wf else None), (rp if fi == d6 else None)
        out["f"][c] = M.f_double(x, u, p, a_ww, a_rp)
        if fi == wf:
            out["xn"][c] = M.erk4(x, u, p, h, a_ww)
            of, oxn, oS = f_under_wrench(orc, x, u, p, ww), rk4_under_wrench(orc, x, u, p, ww, h), None
        else:
            out["xn"][c], out["S"][c] = cache[(x.tobytes(), u.tobytes(), p.tobytes(), h)]
            of = orc.f6(x, u, p, rp)
            oxn, oA, oB = orc.rk4_sens(x, u, p, h, drp=a_rp)
            oS = np.concatenate([oA, oB], axis=1)
        out["e_orc"][c, 0] = scaled_err(of, out["f"][c]).max()
        out["e_orc"][c, 1] = scaled_err(oxn, out["xn"][c]).max()
        if oS is not None:
            out["e_orc"][c, 2] = scaled_err(oS, out["S"][c]).max()
    # the sign-change cases of the kinks family do what they are there for
    k = FAMILIES.index("kinks")
    idx = np.nonzero(out["family"] == k)[0][16:]
    crossed = [(np.sign(out["x"][c, [6, 8, 11]]) * np.sign(out["xn"][c, [6, 8, 11]]) < 0).any() for c in idx]
    assert all(crossed), crossed
    out["E_orc"] = np.array([[np.max(out["e_orc"][out["family"] == fi, q]) for q in range(3)] for fi in range(len(FAMILIES))])
    out["families"] = np.array(FAMILIES)
    return out


def main():
    out = build()
    for fi, fam in enumerate(FAMILIES):
        print(f"{fam:15s} n = {int((out['family'] == fi).sum()):3d}   oracle worst scaled error  f {out['E_orc'][fi, 0]:.2e}  x+ {out['E_orc'][fi, 1]:.2e}"
              f"  S {out['E_orc'][fi, 2]:.2e}   max|S| {np.abs(out['S'][out['family'] == fi]).max():.2e}")
    if "--check" in sys.argv:
        tmp = OUT + ".check"
        save_npz(tmp, out)
        same = open(tmp, "rb").read() == open(OUT, "rb").read()
        os.remove(tmp)
        print("identical to the committed fixture" if same else "DIFFERS from the committed fixture")
        sys.exit(0 if same else 1)
    save_npz(OUT, out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(out['h'])} cases")


if __name__ == "__main__":
    main()
