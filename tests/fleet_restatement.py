"""numpy restatement of the fleet planning tick (include/bluerov2_nmpc.h, brov_fleet_*), the yardstick of
bluerov2_amd/csrc/fleet_kernel.hip.  It is the specification of the segmented select and of the hold / status rule.

A fleet is V vehicles x C candidates over records [V * C]: record v * C + c is candidate c of vehicle v.
  eligible   status == 0 and a finite cost (NaN, +Inf and -Inf never win)
  winner     the eligible candidate of the lowest cost, the lowest index on equal cost (-0.0 == 0.0); -1 when none is eligible
  record     a copy of the winner's 104 bytes, zeros when there is none
  hold       without a winner the vehicle keeps the input it was given last; its status is candidate 0's if that is non-zero, else
             STATUS_NAN (candidate 0 reported success with a cost that is not finite)"""
import numpy as np

RESULT_DTYPE = np.dtype([("u0", "f8", (4,)), ("cost", "f8"), ("kkt", "f8"), ("status", "i4"), ("qp_iter", "i4"), ("thrust", "f8", (6,))])
assert RESULT_DTYPE.itemsize == 104
STATUS_SUCCESS, STATUS_NAN = 0, 1


def select(rec, V, C):
    """(winner [V] int32, winner_rec [V]) of records [V * C]"""
    rec = np.asarray(rec)
    assert rec.dtype == RESULT_DTYPE and rec.shape == (V * C,)
    winner = np.full(V, -1, dtype=np.int32)
    winner_rec = np.zeros(V, dtype=RESULT_DTYPE)
    for v in range(V):
        g = rec[v * C:(v + 1) * C]
        best = -1
        for c in range(C):   # ascending: an equal cost never replaces an earlier index
            if g["status"][c] != STATUS_SUCCESS or not np.isfinite(g["cost"][c]):
                continue
            if best < 0 or g["cost"][c] < g["cost"][best]:
                best = c
        winner[v] = best
        if best >= 0:
            winner_rec[v] = g[best]
    return winner, winner_rec


def apply(rec, V, C, u_hold):
    """what a step gives every vehicle: (winner [V], u [V, 4], status [V]); u_hold [V, 4] = the inputs given last (zeros after a reset)"""
    winner, _ = select(rec, V, C)
    u = np.array(u_hold, dtype=np.float64).reshape(V, 4).copy()
    status = np.zeros(V, dtype=np.int32)
    for v in range(V):
        if winner[v] >= 0:
            u[v] = rec["u0"][v * C + winner[v]]
        else:
            s0 = rec["status"][v * C]
            status[v] = s0 if s0 != STATUS_SUCCESS else STATUS_NAN
    return winner, u, status
