#!/usr/bin/env python3
"""dev tool: dynamic instructions per solve of the headline kernel, ALL classes -- a lone wave pays a four-cycle issue slot for a scalar, an LDS
or a wait instruction as it does for a vector one (profiles/*_fused_issue_slots.txt).  One child run of `bench.py` (headline leg only) under
rocprofv3 --pmc <one group of counters> --kernel-trace per group, nothing else traced; per-launch means over the timed launches, divided by
the launch's waves.  usage: issue_slot_counters.py [kernel name] [bench args...]"""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GROUPS = (("SQ_WAVES", "SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_INSTS_VALU", "SQ_INSTS_MFMA", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_SMEM"),
          ("SQ_WAVES", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_INSTS_BRANCH", "SQ_INSTS_SENDMSG", "SQ_INSTS_FLAT", "SQ_WAIT_INST_ANY", "SQ_WAIT_ANY"))


def main():
    kernel = sys.argv[1] if len(sys.argv) > 1 else "rti_fused_kernel"
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="brov_slots_", dir="/tmp")
    per_wave = {}
    try:
        for n, group in enumerate(GROUPS):
            d = os.path.join(tmp, f"p{n}")
            cmd = [tool, "--pmc", *group, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "c", "--", sys.executable,
                   os.path.join(ROOT, "bench.py"), "--steps", "10", "--warmup", "5", "--full", "--no-cpu-baseline", "--no-extra", "--no-traffic"] + sys.argv[2:]
            r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp", BROV_BENCH_PMC_CHILD="1"), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
            vals = {c: [] for c in group}
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    name = row["Kernel_Name"].split("(")[0].replace("brov::", "").replace("void ", "").strip()
                    if row["Counter_Name"] in vals and name == kernel:
                        vals[row["Counter_Name"]].append(float(row["Counter_Value"]))
            if not vals["SQ_WAVES"]:
                print(f"group {n}: no rows for {kernel} (rc {r.returncode}: {r.stderr.decode(errors='replace')[-400:]})")
                continue
            tail = {c: (v[5:] if len(v) > 5 else v) for c, v in vals.items()}   # the first launches start from a cold iterate
            waves = sum(tail["SQ_WAVES"]) / len(tail["SQ_WAVES"])
            for c in group[1:]:
                if tail[c]:
                    per_wave[c] = sum(tail[c]) / len(tail[c]) / waves
            print(f"group {n}: {len(tail['SQ_WAVES'])} launches of {kernel}, {waves:.0f} waves each")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for c, v in per_wave.items():
        print(f"  {c:20s} {v * (4.0 if c in ('SQ_WAVE_CYCLES', 'SQ_BUSY_CYCLES', 'SQ_WAIT_INST_ANY', 'SQ_WAIT_ANY') else 1.0):12.1f} per wave"
              + ("  (x 4: counted in units of four cycles)" if c == "SQ_WAVE_CYCLES" else ""))
    keys = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_SMEM", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR")
    if all(k in per_wave for k in keys):
        print(f"  sum over classes (VALU incl. MFMA + SALU + LDS + SMEM + VMEM) {sum(per_wave[k] for k in keys):.1f} instructions per solve")


main()
