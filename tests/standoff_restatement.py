"""numpy restatement of the stand-off term of the fleet loop (include/bluerov2_nmpc_standoff.h, brov_standoff_*), the yardstick of
bluerov2_amd/csrc/standoff_kernel.hip and of the walk in bluerov2_amd/csrc/standoff_walk.hpp.  One IEEE double operation per step, in the
order the header fixes; numpy's elementwise products, sums and quotients are each rounded once and never fused.

A fleet is V vehicles x C candidates; instance b = v * C + c.  x [V * C, N + 1, >= 3] are the candidates' predicted paths (the solver's
iterate; columns 0..2 are read).  The scene is the stored triangles st = (v0, e1, e2) of mesh_restatement.stored() (or None) and the boxes
lo, hi [n, 3].
  tri_d2    the squared distance of every point from every stored triangle: the closest point by Voronoi regions, the first rule that holds
  box_d2    e_c = max(max(lo_c - p_c, p_c - hi_c), 0), (e_x^2 + e_y^2) + e_z^2
  s2        per candidate min(reach2, min D2) over the stages first ... N, all triangles and all boxes; the minimum starts at reach2 =
            reach * reach, is updated by D2 < m (a NaN D2 is skipped), and a stage with a NaN coordinate is skipped outright.  This is brute
            force: every point against every triangle.  A minimum of non-NaN values has no order, so the stages, triangles and boxes are
            vectorised (s2_sequential is the same thing written as the loops, for small shapes)
  rescore   the clearance term's rule on s2 (clearance_restatement.rescore)
  stats     last_s2 = s2 of the winner or -1, min_s2 = its running minimum over the steps with a winner, below = steps with s2 < r2"""
import numpy as np

import clearance_restatement as CR
from mesh_restatement import stored  # noqa: F401  (the stored form of triangles [T, 3, 3]: what callers pass as st)

rescore = CR.rescore


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def tri_d2(p, st):
    """[P, T]: D2 of the points p [P, 3] from the stored triangles st = (v0, e1, e2), each [T, 3]"""
    v0, e1, e2 = (np.asarray(q, dtype=np.float64) for q in st)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = p - v0
        b = a - e1
        c = a - e2
        d1, d2, d3, d4, d5, d6 = _dot(e1, a), _dot(e2, a), _dot(e1, b), _dot(e2, b), _dot(e1, c), _dot(e2, c)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        g, h = d4 - d3, d5 - d6
        rule = np.select([(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                          (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (g >= 0) & (h >= 0)], [1, 2, 3, 4, 5, 6], default=7)
        # at most one quotient per rule: the operands are selected, the quotient is the rule's own
        num = np.select([rule == 3, rule == 5, rule == 6, rule == 7], [d1, d2, g, np.ones_like(d1)], default=0.0)
        den = np.select([rule == 3, rule == 5, rule == 6, rule == 7], [d1 - d3, d2 - d6, g + h, (va + vb) + vc], default=1.0)
        q = num / den
        s = np.select([rule == 2, rule == 3, rule == 6, rule == 7], [np.ones_like(q), q, 1.0 - q, vb * q], default=0.0)
        t = np.select([rule == 4, (rule == 5) | (rule == 6), rule == 7], [np.ones_like(q), q, vc * q], default=0.0)
        r = (a - s[..., None] * e1) - t[..., None] * e2
        return _dot(r, r)


def tri_d2_one(p, v0, e1, e2):
    """(D2, rule) of ONE point and ONE stored triangle, written as the rules read: python floats, one operation per step"""
    p, v0, e1, e2 = ([float(z) for z in q] for q in (p, v0, e1, e2))
    f = np.float64
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = [f(p[j]) - f(v0[j]) for j in range(3)]
        b = [a[j] - f(e1[j]) for j in range(3)]
        c = [a[j] - f(e2[j]) for j in range(3)]
        dot = lambda u, w: (f(u[0]) * f(w[0]) + f(u[1]) * f(w[1])) + f(u[2]) * f(w[2])    # noqa: E731
        d1, d2, d3, d4, d5, d6 = dot(e1, a), dot(e2, a), dot(e1, b), dot(e2, b), dot(e1, c), dot(e2, c)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        g, h = d4 - d3, d5 - d6
        if d1 <= 0 and d2 <= 0:
            rule, s, t = 1, f(0), f(0)
        elif d3 >= 0 and d4 <= d3:
            rule, s, t = 2, f(1), f(0)
        elif vc <= 0 and d1 >= 0 and d3 <= 0:
            rule, s, t = 3, d1 / (d1 - d3), f(0)
        elif d6 >= 0 and d5 <= d6:
            rule, s, t = 4, f(0), f(1)
        elif vb <= 0 and d2 >= 0 and d6 <= 0:
            rule, s, t = 5, f(0), d2 / (d2 - d6)
        elif va <= 0 and g >= 0 and h >= 0:
            w = g / (g + h)
            rule, s, t = 6, f(1) - w, w
        else:
            den = f(1) / ((va + vb) + vc)
            rule, s, t = 7, vb * den, vc * den
        r = [(a[j] - s * f(e1[j])) - t * f(e2[j]) for j in range(3)]
        return dot(r, r), rule


def box_d2(p, lo, hi):
    """[P, n]: D2 of the points p [P, 3] from the boxes lo, hi [n, 3]; 0 inside"""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1, 3), np.asarray(hi, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.maximum(np.maximum(lo - p, p - hi), 0.0)
        return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def point_min(p, st=None, lo=(), hi=(), chunk=2048):
    """[P]: the minimum of D2 over all triangles and boxes for every point, +Inf over an empty set; a NaN D2 is skipped, and so is (+Inf) a
    point with a NaN coordinate"""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    out = np.full(len(p), np.inf)
    for i in range(0, len(p), chunk):
        q = p[i:i + chunk]
        cols = []
        if st is not None and len(st[0]):
            cols.append(tri_d2(q, st))
        if len(np.asarray(lo).reshape(-1, 3)):
            cols.append(box_d2(q, lo, hi))
        if cols:
            d = np.concatenate(cols, axis=1)
            d = np.where(np.isnan(d), np.inf, d)
            out[i:i + chunk] = d.min(axis=1)
    out[np.isnan(p).any(axis=1)] = np.inf
    return out


def fold(pm, first, reach):
    """s2 [B] from the per-point minima pm [B, N + 1]: min(reach2, min over the stages first ... N)"""
    reach2 = np.float64(reach) * np.float64(reach)
    return np.minimum(reach2, np.asarray(pm, dtype=np.float64)[:, first:].min(axis=1))


def s2(x, first, reach, st=None, lo=(), hi=()):
    x = np.asarray(x, dtype=np.float64)
    B, K = x.shape[:2]
    assert 0 <= first <= K - 1
    return fold(point_min(x[:, :, :3].reshape(-1, 3), st, lo, hi).reshape(B, K), first, reach)


def s2_sequential(x, first, reach, st=None, lo=(), hi=()):
    """s2 as the header words it: one running minimum per candidate, started at reach2, over stages, boxes and triangles in turn"""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1, 3), np.asarray(hi, dtype=np.float64).reshape(-1, 3)
    reach2 = np.float64(reach) * np.float64(reach)
    out = np.empty(len(x))
    for b in range(len(x)):
        m = reach2
        for k in range(first, x.shape[1]):
            p = x[b, k, :3]
            if np.isnan(p).any():
                continue
            for j in range(len(lo)):
                d = box_d2(p, lo[j], hi[j])[0, 0]
                if d < m:
                    m = d
            for j in range(len(st[0]) if st is not None else 0):
                d, _ = tri_d2_one(p, st[0][j], st[1][j], st[2][j])
                if d < m:
                    m = d
        out[b] = m
    return out


def fresh_stats(V):
    return dict(last_s2=np.full(V, -1.0), min_s2=np.full(V, np.inf), below=np.zeros(V, dtype=np.int32))


def stats(st, s2v, winner, V, C, radius):
    """the statistics after a step, from those before it"""
    st = {k: a.copy() for k, a in st.items()}
    r2 = np.float64(radius) * np.float64(radius)
    for v in range(V):
        if winner[v] >= 0:
            d = s2v[v * C + winner[v]]
            st["last_s2"][v] = d
            if d < st["min_s2"][v]:
                st["min_s2"][v] = d
            if d < r2:
                st["below"][v] += 1
        else:
            st["last_s2"][v] = -1.0
    return st
