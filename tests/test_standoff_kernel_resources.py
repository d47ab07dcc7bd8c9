"""The stand-off kernels in the build's own resource report (bluerov2_amd/lib/obj/standoff_kernel.resources.txt, written by the Makefile's
rule): no scratch and no VGPR spill in either, and no LDS -- the walk over the hierarchy is forward only, so there is no stack --; registers
and occupancy are printed, and recorded in DESIGN.md section 4.12d, not fixed in advance."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = (r"\d+standoff_dist_kernelE", r"\d+standoff_stats_kernelE")


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


def test_the_kernels_use_no_scratch():
    rep = _report("standoff_kernel")
    assert len(rep) == len(KERNELS), sorted(rep)                  # the file holds these kernels and nothing else
    for pat in KERNELS:
        hit = [r for n, r in rep.items() if re.search(pat, n)]
        assert len(hit) == 1, (pat, sorted(rep))
        k = hit[0]
        print(pat, "VGPRs", k["VGPRs"], "AGPRs", k["AGPRs"], "SGPRs", k["TotalSGPRs"], "occupancy", k["Occupancy"], "LDS", k["LDS Size"],
              "SGPRs kept in VGPR lanes", k["SGPRs Spill"])
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (pat, k)
        assert k["LDS Size"] == 0, (pat, k)


def test_the_makefile_gates_the_new_kernels():
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "standoff_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/standoff_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    assert "standoff_kernel.resources.txt" in rule and "standoff_dist_kernel|standoff_stats_kernel" in rule
    assert "standoff_walk.hpp" in rule and "mesh_bvh.hpp" in rule and "bluerov2_nmpc_standoff.h" in rule
    assert "standoff_kernel.hpp" in mk[mk.index("$(OUTDIR)/obj/fleet_api.o:"):].splitlines()[0]
    assert "standoff_kernel.hpp" in mk[mk.index("$(OUTDIR)/obj/nmpc_api.o:"):].splitlines()[0]
