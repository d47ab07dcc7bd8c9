"""The one-wave fused kernels (rti_fused_kernel, rti_fused_kernel_grid; 12 <= N <= 23) against THEIR OWN outputs as recorded from the parent of
the commit that cut the early-exit path's issue slots: work on instruction counts must leave every FP64 operation, its operands and its place in
its dependency chain alone, so records and iterates are the same bits.  64 instances (one wave each), 3 steps of solve() on the circle window at
the ends of the one-wave range and at the flagship horizon; a quarter of the instances saturated (bench.saturate), so the QP loop, the active-set
tries and the checkpointed sweep run next to the early exit; one case on a general grid, one with the 6-disturbance model.

The fixtures hold nothing but this library's outputs: tests/golden/fused_parent_outputs.<case>.npz, one file per case (together they are past
what one committed file may hold), the result records of every step and the iterate after the last one (the iterates of the steps before are
the inputs of the records that follow them).  Recorded with
    python tests/test_gpu_fused_bitwise.py --record
on a build of the commit to compare against; the file's tests then pass trivially on that build."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
B, STEPS = 64, 3
RECORD_FIELDS = ("u0", "cost", "kkt", "status", "qp_iter", "thrust")
ITERATE_FIELDS = ("x", "u", "pi", "lam")
CASES = {"N14": (14, None), "N20": (20, None), "N23": (23, None), "N20_grid": (20, "grid"), "N20_dist6": (20, "dist6")}


def _fixture(case):
    return os.path.join(HERE, "golden", f"fused_parent_outputs.{case}.npz")


def _run(ba, case):
    """{"<step>/<field>": array} of the case: the records of every step, the iterate after the last"""
    from bench import synthetic_inputs, saturate, step_outputs
    N, variant = CASES[case]
    x0, circ = synthetic_inputs(B, seed=300 + N)
    x0 = saturate(x0, 0.25, seed=301 + N)
    s = ba.BatchSolver(B, ba.SolverOptions(N, 1.0 / N))
    s.set_x0(x0); s.set_params(ba.P_NOMINAL)
    if variant == "grid":
        s.set_time_steps(1.0 / N * 1.01 ** np.arange(N))
    if variant == "dist6":
        s.enable_dist6()
        s.set_rp_disturbance(np.random.default_rng(302).uniform(-2.0, 2.0, (B, N + 1, 2)))
    out = {}
    n_qp = 0
    for k in range(STEPS):
        s.set_yref(circ[k:k + N + 1])
        s.solve(sync=True)
        assert s.last_kernel_path() == ba.PATH_FUSED
        o = step_outputs(s, s.results())
        n_qp += int((o["qp_iter"] > 0).sum())
        for f in RECORD_FIELDS + (ITERATE_FIELDS if k == STEPS - 1 else ()):
            out[f"{k}/{f}"] = o[f]
    s.close()
    return out, n_qp


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import bluerov2_amd
    return bluerov2_amd


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_outputs_are_the_parents_bit_for_bit(ba, case):
    want = np.load(_fixture(case))
    got, n_qp = _run(ba, case)
    assert sorted(want.files) == sorted(got)
    # the batch is the mixed one: early exits and interior-point solves side by side
    assert 0 < n_qp < STEPS * B
    bad = [k for k in want.files if not np.array_equal(want[k], got[k], equal_nan=True)]
    for k in bad:
        d = want[k] != got[k]
        print(f"{case} {k}: {int(d.sum())} of {d.size} elements differ, max |diff| {np.nanmax(np.abs(want[k] - got[k])):.3e}")
    assert not bad, (case, bad)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    sys.path.insert(0, os.path.dirname(HERE))
    import bluerov2_amd
    for c in sorted(CASES):
        arrs, n = _run(bluerov2_amd, c)
        np.savez_compressed(_fixture(c), **arrs)
        print(f"{c}: {os.path.getsize(_fixture(c))} bytes, {n} interior-point solves in {STEPS} steps")
