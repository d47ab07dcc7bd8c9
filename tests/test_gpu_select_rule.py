"""The one select rule of bluerov2_amd/csrc/select_device.hpp -- eligible is status SUCCESS and a finite cost; the lowest cost wins, the
lowest index on equal cost; -1 when nobody is eligible -- in the block kernels that stand on it: select_best_kernel (BatchSolver.select_best)
and group_select_kernel / group_pack_kernel (SolverGroup, both gather modes, W ranks on one device through the copy collective).

Every case plants synthetic records in the solvers' own record arrays behind a solve and asks for the winner.  What is expected comes from
fleet_restatement.select(records, 1, n), the specification, never from another kernel.  (The fleet's kernel is held to the same
specification in tests/test_gpu_fleet.py.)"""
import numpy as np
import pytest

import fleet_restatement as FR
from test_gpu_fleet import synthetic_records

pytestmark = pytest.mark.gpu
N, TS = 20, 0.05
MODES = ("GATHER_RECORDS", "GATHER_PACKED")
# (ranks, instances): even and uneven shards, one and two select blocks (1025 slots is the smallest case that takes the ticket path),
# a slot count that is no multiple of 64
GROUPS = [(1, 257), (1, 1025), (2, 130), (3, 1027), (4, 2051)]


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


def families(n, seed):
    """(name, records [n], the winner where the construction fixes it, else None), in the style of
    test_gpu_fleet.py::test_select_equals_the_restatement_byte_for_byte"""
    r = synthetic_records(1, n, seed)
    yield "mixed costs, 20 % failed", r, None
    q = r.copy(); q["status"] = 0; q["cost"] = -0.5
    yield "all equal", q, 0
    q = r.copy(); q["status"] = 4; q["status"][n - 1] = 0; q["cost"][n - 1] = 3.0
    yield "the only eligible record last", q, n - 1
    q = r.copy(); q["status"] = 2
    yield "none eligible", q, -1
    q = r.copy(); q["status"] = 0
    q["cost"][0::3] = np.nan; q["cost"][1::3] = np.inf; q["cost"][2::3] = -np.inf
    yield "NaN, +Inf and -Inf with status 0", q, -1
    q = q.copy(); q["cost"][n // 2] = 7.0
    yield "... and one finite record", q, n // 2
    q = r.copy(); q["status"] = 0; q["cost"] = np.abs(q["cost"]) + 1.0
    q["cost"][n - 1] = -1e9; q["status"][n - 1] = 3
    yield "the lowest cost carried by a failed record", q, None


def expected(q, fixed):
    want = int(FR.select(q, 1, len(q))[0][0])
    assert fixed is None or want == fixed
    return want


def plant(solver, q):
    """q into the solver's own record array, through a zero-copy view of it"""
    import torch
    from bluerov2_amd import distributed as D
    assert len(q) == solver.B
    D.records_tensor_from_solver(solver).copy_(torch.from_numpy(np.frombuffer(q.tobytes(), dtype=np.uint8).copy()))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 650])
def test_select_best_is_the_restatement(ba, n):
    import torch
    s = ba.BatchSolver(n, ba.SolverOptions(N, TS))
    s.set_params(ba.P_NOMINAL)
    s.solve(sync=True)
    for name, q, fixed in families(n, seed=7 * n):
        want = expected(q, fixed)
        plant(s, q)
        torch.cuda.synchronize()
        idx, rec = s.select_best()
        print(f"[select_best n={n}] {name}: {idx}, expected {want}")
        assert idx == want, (n, name)
        assert want < 0 or rec.tobytes() == q[want].tobytes(), (n, name)
    if n > 1:
        assert expected(q, None) != n - 1          # (the last family: the failed record carries the lowest cost and does not win)
    s.close()


@pytest.fixture(scope="module")
def group_of(ba):
    """SolverGroup(W ranks on device 0, copy collective) behind one solve, made once per (W, total)"""
    made = {}

    def get(W, total):
        if (W, total) not in made:
            g = ba.SolverGroup([0] * W, total, ba.SolverOptions(N, TS), collective="copy")
            g.set_params(ba.P_NOMINAL); g.solve(); g.synchronize()
            made[(W, total)] = g
        return made[(W, total)]

    yield get
    for g in made.values():
        g.close()


def group_select(ba, g, q, mode):
    """q planted shard by shard, gathered with `mode`, selected"""
    import torch
    g.synchronize()                                 # the pulls of the gather before have read the records they share
    for shard, (lo, hi) in zip(g.shards, g.bounds):
        plant(shard, q[lo:hi])
    torch.cuda.synchronize()
    g.gather(getattr(ba, mode))
    return g.select_best()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,total", GROUPS)
def test_group_select_is_the_restatement(ba, group_of, W, total, mode):
    g = group_of(W, total)
    assert [hi - lo for lo, hi in g.bounds] == [total // W + (1 if r < total % W else 0) for r in range(W)]
    for name, q, fixed in families(total, seed=W + total):
        want = expected(q, fixed)
        idx, rec = group_select(ba, g, q, mode)
        print(f"[group W={W} total={total} {mode}] {name}: {idx}, expected {want}")
        assert idx == want, (W, total, mode, name)
        assert (rec is None) if want < 0 else (rec.tobytes() == q[want].tobytes()), (W, total, mode, name)


@pytest.mark.parametrize("W,total", GROUPS)
def test_infinite_costs_win_nowhere_in_a_shard(ba, group_of, W, total):
    """Nothing but +Inf with status 0 is left to choose from in the last shard, every other record has failed: no winner, wherever the
    infinities sit -- the first slot of the shard, the last, one behind the first pass of the block (slot >= 256, where the shard has one),
    or all of them.  (Before the rule was one, a scanning thread took +Inf as its first eligible record and no later one.)"""
    g = group_of(W, total)
    lo, hi = g.bounds[-1]
    base = synthetic_records(1, total, seed=total); base["status"] = 4
    places = {"first": [lo], "last": [hi - 1], "whole shard": list(range(lo, hi))}
    if hi - lo > 256:
        places["slot 256"] = [lo + 256]
    for where, at in places.items():
        q = base.copy(); q["status"][at] = 0; q["cost"][at] = np.inf
        assert expected(q, -1) == -1
        for mode in MODES:
            idx, rec = group_select(ba, g, q, mode)
            print(f"[group W={W} total={total} {mode}] +Inf at {where}: {idx}")
            assert idx == -1 and rec is None, (W, total, mode, where)
