"""The error-state filter's kernels in the build's own resource report (bluerov2_amd/lib/obj/eskf_kernel.resources.txt, written by the Makefile's
rule for eskf_kernel.o): no scratch, and the registers, LDS and occupancy DESIGN.md section 4.4b claims.  Beside tests/test_kernel_resources.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_FILTER = (21 * 21 + 12 * 12 + 21 + 22 + 12) * 8      # P, the factor of S, dx, the predicted state, the innovation
FILTERS_PER_WAVE = 2


def _report():
    import bluerov2_amd
    bluerov2_amd.build_library()
    txt = open(os.path.join(ROOT, "bluerov2_amd", "lib", "obj", "eskf_kernel.resources.txt")).read()
    rep, name = {}, None
    for ln in txt.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            rep[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and name:
            rep[name][m.group(1).strip()] = int(m.group(2))
    return rep


def _one(rep, pat):
    hit = [r for n, r in rep.items() if re.search(pat, n)]
    assert len(hit) == 1, (pat, sorted(rep))
    return hit[0]


def test_no_scratch_and_the_claimed_occupancy():
    rep = _report()
    upd, pred = _one(rep, r"eskf_tick_kernelILb1E"), _one(rep, r"eskf_tick_kernelILb0E")
    for k in (upd, pred, _one(rep, r"eskf_inputs_from_solver_kernel"), _one(rep, r"eskf_apply_kernel")):
        print(k)
        assert k["ScratchSize"] == 0, k
    for k in (upd, pred):
        assert k["LDS Size"] == FILTERS_PER_WAVE * LDS_PER_FILTER, k
        assert k["VGPRs"] + k["AGPRs"] <= 256 and k["Occupancy"] >= 2, k      # two waves per SIMD, eight per CU: 80 KB of the CU's 160 KB LDS
        assert 8 * k["LDS Size"] <= 160 * 1024
    assert _one(rep, r"eskf_inputs_from_solver_kernel")["LDS Size"] == 0 and _one(rep, r"eskf_apply_kernel")["LDS Size"] == 0


def test_makefile_gates_the_new_object():
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "eskf_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/eskf_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    for k in ("eskf_tick_kernel", "eskf_inputs_from_solver_kernel", "eskf_apply_kernel"):
        assert k in rule
