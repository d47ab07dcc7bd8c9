"""Static instruction totals of the loops on rti_fused_kernel's early-exit path -- the two column loops of the linearisation, the step-0
factor loop, the forward loop and the adjoint loop with commit -- read out of the built object through scripts/dev/isa_path.py.  One wave per
SIMD: every instruction of these loops, whatever its class, is a four-cycle issue slot times the loop's trips (profiles/issue_slots_*.txt), so
a change that quietly gives slots back shows here before it shows in a benchmark.  The budgets are the counts of the build that introduced
this file; a loop may get shorter, and then its budget should follow it down.

Needs the object the library was linked from (bluerov2_amd/lib/obj/qp_kernel.o, left there by the build) and the toolchain's disassembler."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bluerov2_amd", "lib", "obj", "qp_kernel.o")
# instructions per trip (a sweep trip holds three stages), MFMAs among them
BUDGET = {"general columns": (1207, 0), "closed-form columns": (523, 0), "factor (step 0)": (568, 27), "forward": (170, 0), "adjoint + commit": (147, 0)}


@pytest.fixture(scope="module")
def early_exit_loops():
    if not os.path.exists(OBJ):
        pytest.skip("bluerov2_amd/lib/obj/qp_kernel.o is not there: the library has not been built in this tree")
    sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
    import isa_path
    name, ins, loops = isa_path.loops(OBJ)
    assert "rti_fused_kernel" in name
    return loops


@pytest.mark.parametrize("loop", sorted(BUDGET))
def test_loop_stays_inside_its_issue_budget(early_exit_loops, loop):
    start, end, classes = early_exit_loops[loop]
    total, mfma = BUDGET[loop]
    print(f"{loop}: {end - start} instructions (budget {total}), {classes['mfma']} MFMA; " + " ".join(f"{c}={v}" for c, v in sorted(classes.items())))
    assert classes["mfma"] == mfma          # the arithmetic itself is not what this file budgets: it must not move at all
    assert end - start <= total


def test_fp64_arithmetic_of_the_sweeps_is_what_it_was(early_exit_loops):
    """per trip of three stages: 189 FP64 operations in the factor loop, 48 DPP multiply-adds + 12 additions forward, 30 operations in the adjoint"""
    fac, fwd, adj = (early_exit_loops[k][2] for k in ("factor (step 0)", "forward", "adjoint + commit"))
    assert fac["f64"] == 189 and (fwd["f64 dpp"], fwd["f64"]) == (48, 12) and adj["f64"] == 30
