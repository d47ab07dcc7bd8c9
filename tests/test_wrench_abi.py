"""The world-frame wrench of the plant and the on-device DOB loop at the ABI level, without a GPU: the header declares the entry
points, the cross-compiled library exports them, and plant_wrench_kernel holds its state in registers (no scratch)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["brov_plant_wrench_constant_host", "brov_plant_wrench_periodic", "brov_plant_wrench_table_host", "brov_plant_wrench_off",
           "brov_plant_wrench_mode", "brov_plant_wrench_seek", "brov_plant_wrench_tick", "brov_plant_wrench_eval_host",
           "brov_closed_loop_ex", "brov_closed_loop_dob"]


def _header():
    txt = open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_wrench_api_and_the_dob_loop():
    txt = _header()
    declared = set(re.findall(r"\b(brov_[a-z0-9_]+)\s*\(", txt))
    assert not [n for n in SYMBOLS if n not in declared]
    modes = dict(re.findall(r"#define (BROV_WRENCH_[A-Z]+) (\d+)", txt))
    assert modes == {"BROV_WRENCH_OFF": "0", "BROV_WRENCH_CONSTANT": "1", "BROV_WRENCH_PERIODIC": "2", "BROV_WRENCH_TABLE": "3"}
    # the signatures the issue fixes: the seed is 64 bits wide, the tick counter signed 64 bits
    assert re.search(r"int\s+brov_plant_wrench_periodic\(brov_solver\*\s*s,\s*uint64_t seed,\s*double scale,\s*double phase0,\s*double dphi,\s*double tz_div\)", txt)
    assert re.search(r"int64_t\s+brov_plant_wrench_tick\(const brov_solver\*", txt)
    assert re.search(r"int\s+brov_plant_wrench_seek\(brov_solver\*\s*s,\s*int64_t tick\)", txt)
    # brov_closed_loop keeps its signature
    assert re.search(r"int brov_closed_loop\(brov_solver\* s, int ticks, int line0, int ncols, double dt, int substeps, double\* u_log, double\* x_log,\s*"
                     r"int32_t\* st_log\);", txt)


def test_library_exports_the_wrench_api_and_the_dob_loop():
    import bluerov2_amd
    bluerov2_amd.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", bluerov2_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split())
    assert not [n for n in SYMBOLS if n not in exported]


def test_python_mirror_names_the_modes():
    import bluerov2_amd as ba
    assert (ba.WRENCH_OFF, ba.WRENCH_CONSTANT, ba.WRENCH_PERIODIC, ba.WRENCH_TABLE) == (0, 1, 2, 3)
    for name in ("set_plant_wrench", "plant_wrench_off", "plant_wrench", "plant_wrench_seek", "plant_wrench_tick", "closed_loop_dob"):
        assert callable(getattr(ba.BatchSolver, name))


def test_plant_wrench_kernel_uses_no_scratch():
    """the backend's own resource report of plant_wrench.hip (device-only compile): its kernels, plant_kernel among them, without scratch;
    the plant kernels at no more than 256 registers (measured: 204), so that two waves per SIMD stay resident as the backend reports today"""
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "plant_wrench.hip"], capture_output=True,
                         text=True, timeout=600).stdout
    rep = {}
    for ln in out.splitlines():
        m = re.match(r"Name: (\S+)", ln)
        if m:
            rep[m.group(1)] = {k: int(v) for k, v in re.findall(r"\|([A-Za-z ]+): (\d+)", ln)}
    for short in ("plant_kernel", "plant_wrench_kernel", "wrench_eval_kernel"):
        hit = [r for m, r in rep.items() if re.search(r"\d+%sE" % short, m)]
        assert len(hit) == 1, (short, sorted(rep))
        assert hit[0]["scratch"] == 0, (short, hit[0])
        assert hit[0]["VGPRs"] <= 256 and hit[0]["occ"] >= 2, (short, hit[0])


def test_makefile_gates_the_plant_wrench_kernel_on_scratch():
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "plant_wrench.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/plant_wrench.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "plant_wrench_kernel" in rule and "rm -f $@" in rule
