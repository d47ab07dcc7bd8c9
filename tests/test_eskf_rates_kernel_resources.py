"""The masked filter tick and the IMU/GPS stage's kernels in the build's own resource reports (bluerov2_amd/lib/obj/*.resources.txt, written
by the Makefile's rules): what DESIGN.md sections 4.4c and 4.9h claim.  Beside tests/test_eskf_kernel_resources.py, which holds the two
existing instantiations of the tick."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_FILTER = (21 * 21 + 12 * 12 + 21 + 22 + 12) * 8      # P, the factor of S, dx, the predicted state, the innovation
FILTERS_PER_WAVE = 2


def _report(obj):
    import bluerov2_amd
    bluerov2_amd.build_library()
    txt = open(os.path.join(ROOT, "bluerov2_amd", "lib", "obj", obj + ".resources.txt")).read()
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


def _rule(mk, obj):
    rule = mk[mk.index("$(OUTDIR)/obj/" + obj + ".o:"):]
    return rule[:rule.index("\n\n")]


def test_the_masked_tick_meets_what_the_update_tick_claims():
    rep = _report("eskf_kernel")
    k = _one(rep, r"\d+eskf_tick_masked_kernelE")
    print(k)
    assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, k
    assert k["LDS Size"] == FILTERS_PER_WAVE * LDS_PER_FILTER == 10240, k
    assert k["VGPRs"] + k["AGPRs"] <= 256 and k["Occupancy"] >= 2, k
    h = _one(rep, r"\d+eskf_inputs_from_imu_kernelE")
    assert h["ScratchSize"] == 0 and h["LDS Size"] == 0, h
    # its own name: the two existing instantiations keep theirs, one hit each
    assert len([n for n in rep if re.search(r"eskf_tick_kernelILb[01]E", n)]) == 2


def test_the_imu_kernels_use_no_scratch_and_no_lds():
    rep = _report("imu_kernel")
    for pat in (r"\d+imu_measure_kernelE", r"\d+imu_eval_kernelE"):
        k = _one(rep, pat)
        print(pat, k)
        assert k["ScratchSize"] == 0 and k["LDS Size"] == 0 and k["VGPRs Spill"] == 0, (pat, k)
        assert k["VGPRs"] + k["AGPRs"] <= 128 and k["Occupancy"] >= 4, (pat, k)


def test_the_makefile_gates_the_new_kernels():
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    srcs = mk.split("SRCS")[1].splitlines()[0]
    assert "imu_kernel.hip" in srcs and "eskf_kernel.hip" in srcs
    eskf = _rule(mk, "eskf_kernel")
    assert "kernel-resource-usage" in eskf and "ScratchSize" in eskf and "rm -f $@" in eskf
    assert "eskf_tick_masked_kernel" in eskf and "eskf_inputs_from_imu_kernel" in eskf and "eskf_tick_body.inc" in eskf
    imu = _rule(mk, "imu_kernel")
    assert "kernel-resource-usage" in imu and "ScratchSize" in imu and "rm -f $@" in imu
    assert "imu_measure_kernel" in imu and "imu_eval_kernel" in imu
