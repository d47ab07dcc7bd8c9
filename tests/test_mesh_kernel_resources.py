"""The mesh kernels in the build's own resource report (bluerov2_amd/lib/obj/mesh_kernel.resources.txt, written by the Makefile's rule): no
scratch and no VGPR spill in either, as DESIGN.md section 4.9k claims -- the walk over the hierarchy is forward only, so there is no stack to
spill --; registers and occupancy are printed, and recorded there, not fixed in advance."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = (r"\d+mesh_eval_kernelE", r"\d+inspect_mesh_tick_kernelE")


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


def test_the_two_kernels_use_no_scratch():
    rep = _report("mesh_kernel")
    for pat in KERNELS:
        hit = [r for n, r in rep.items() if re.search(pat, n)]
        assert len(hit) == 1, (pat, sorted(rep))
        k = hit[0]
        print(pat, "VGPRs", k["VGPRs"], "AGPRs", k["AGPRs"], "SGPRs", k["TotalSGPRs"], "occupancy", k["Occupancy"], "LDS", k["LDS Size"],
              "SGPRs kept in VGPR lanes", k["SGPRs Spill"])
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0, (pat, k)
        assert k["LDS Size"] == 0, (pat, k)            # no stack: the skip links make the walk a loop over one index


def test_the_makefile_gates_the_new_kernels():
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "mesh_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/mesh_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "rm -f $@" in rule
    assert "mesh_kernel.resources.txt" in rule and "mesh_eval_kernel|inspect_mesh_tick_kernel" in rule
    assert "bluerov2_nmpc_mesh.h" in rule and "range_device.hpp" in rule and "mesh_bvh.hpp" in rule
    inspect_rule = mk[mk.index("$(OUTDIR)/obj/inspect_kernel.o:"):].splitlines()[0]
    assert "range_device.hpp" in inspect_rule                      # the shared bodies rebuild both objects
    assert "mesh_source.hpp" in mk[mk.index("$(OUTDIR)/obj/nmpc_api.o:"):].splitlines()[0]
