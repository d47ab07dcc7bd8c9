"""numpy restatement of the inter-vehicle clearance term of the fleet loop (include/bluerov2_nmpc.h, brov_clearance_*), the yardstick of
bluerov2_amd/csrc/clearance_kernel.hip.  Written sequentially, one IEEE double operation per step, in the order the header fixes.

A fleet is V vehicles x C candidates; instance b = v * C + c.  x [V * C, N + 1, >= 3] are the candidates' predicted paths (the solver's
iterate; columns 0..2 are read), plan [V, N + 1, 3] the positions of the path every vehicle committed to last.
  d2min     per candidate the minimum over the peers w != v and the stages k of ((dx*dx + dy*dy) + dz*dz), d = x[b][k] - plan[w][min(k + shift, N)];
            starts at +Inf, updated by d2 < m (a NaN distance is skipped); +Inf when V == 1
  rescore   a copy of the records with cost += weight * (r2 - d2min) where d2min < r2; a cost that is NaN already keeps its bytes, a NaN the
            sum generates (-Inf + Inf) is written as the quiet NaN 0x7ff8000000000000 (IEEE leaves the sign of a generated NaN open; it is
            the negative one on x86)
  publish   with a winner the plan is the winner's path, without one the old plan advanced by `shift` stages
  stats     last_d2 = d2min of the winner or -1, min_d2 = its running minimum over the steps with a winner, below = steps with d2min < r2"""
import numpy as np

from fleet_restatement import RESULT_DTYPE

QUIET_NAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]


def d2min(x, plan, V, C, shift):
    x, plan = np.asarray(x, dtype=np.float64), np.asarray(plan, dtype=np.float64)
    N = plan.shape[1] - 1
    assert plan.shape == (V, N + 1, 3) and x.shape[:2] == (V * C, N + 1) and 0 <= shift <= N
    out = np.full(V * C, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(V * C):
            v = b // C
            m = np.float64(np.inf)
            for w in range(V):
                if w == v:
                    continue
                for k in range(N + 1):
                    q = plan[w, min(k + shift, N)]
                    dx, dy, dz = x[b, k, 0] - q[0], x[b, k, 1] - q[1], x[b, k, 2] - q[2]
                    d2 = (dx * dx + dy * dy) + dz * dz
                    if d2 < m:
                        m = d2
            out[b] = m
    return out


def rescore(rec, d2, radius, weight):
    """the re-scored copy of records [B] given d2min [B]; r2 = radius * radius is formed once"""
    rec = np.asarray(rec)
    assert rec.dtype == RESULT_DTYPE and rec.shape == np.shape(d2)
    out = rec.copy()
    r2 = np.float64(radius) * np.float64(radius)
    weight = np.float64(weight)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(rec.size):
            if d2[b] < r2:
                gap = r2 - np.float64(d2[b])
                pen = weight * gap
                if np.isnan(rec["cost"][b]):
                    continue                             # a NaN cost keeps its bytes
                cost = np.float64(rec["cost"][b]) + pen
                out["cost"][b] = QUIET_NAN if np.isnan(cost) else cost
    return out


def publish(plan, x, winner, V, C, shift):
    """the plan after a step with the winners `winner` [V] (-1: none)"""
    plan = np.array(plan, dtype=np.float64)
    N = plan.shape[1] - 1
    for v in range(V):
        if winner[v] >= 0:
            plan[v] = np.asarray(x)[v * C + winner[v], :, :3]
        else:
            for k in range(N + 1):           # ascending: reads at or ahead of where it writes
                plan[v, k] = plan[v, min(k + shift, N)]
    return plan


def fresh_stats(V):
    return dict(last_d2=np.full(V, -1.0), min_d2=np.full(V, np.inf), below=np.zeros(V, dtype=np.int32))


def stats(st, d2, winner, V, C, radius):
    """the statistics after a step, from those before it"""
    st = {k: a.copy() for k, a in st.items()}
    r2 = np.float64(radius) * np.float64(radius)
    for v in range(V):
        if winner[v] >= 0:
            d = d2[v * C + winner[v]]
            st["last_d2"][v] = d
            if d < st["min_d2"][v]:
                st["min_d2"][v] = d
            if d < r2:
                st["below"][v] += 1
        else:
            st["last_d2"][v] = -1.0
    return st


def d2min_fast(x, plan, V, C, shift):
    """the same numbers with the peers and stages vectorised: every distance is formed by the same operations in the same order and a
    minimum of non-NaN values has no order, so the bytes are those of d2min (tests hold the two against each other on small shapes)"""
    x, plan = np.asarray(x, dtype=np.float64), np.asarray(plan, dtype=np.float64)
    N = plan.shape[1] - 1
    ks = np.minimum(np.arange(N + 1) + shift, N)
    q = plan[:, ks, :]                                   # [V, N + 1, 3]
    out = np.full(V * C, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(V * C):
            v = b // C
            d = x[b, None, :, :3] - q                    # [V, N + 1, 3]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            d2[v] = np.inf
            d2 = np.where(np.isnan(d2), np.inf, d2)
            out[b] = d2.min() if V > 1 else np.inf
    return out
