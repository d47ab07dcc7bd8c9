#!/usr/bin/env python3
"""compare_device_code.py A B -- are the gfx950 code objects bundled in two host objects / libraries the same code?
Prints, per kernel symbol, instruction count and a hash of its disassembly (addresses stripped) for both files and the verdict.
Used in round 5 to show that cutting qp_kernel.hip into qp/*.hpp changed no instruction (profiles/r5_split_isa.txt)."""
import hashlib
import re
import sys
import os

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import check_exec_restore as C


def kernels(path):
    C.OBJDUMP = C.find_objdump()
    out, name, body = {}, None, []
    for ln in C.listing(path):
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", ln)
        if m:
            if name and not name.startswith("L"):
                out[name] = body
            elif name:                       # a label inside the current function
                body_prev.append(ln.split("<")[1]); name, body = name_prev, body_prev
            name_prev, body_prev = name, body
            if not m.group(1).startswith("L"):
                name, body = m.group(1), []
                name_prev, body_prev = name, body
            continue
        t = ln.split("//")[0].strip()
        if name and t and "file format" not in t:   # (the header of the next code object's listing names a temporary file)
            body.append(t)
    if name:
        out[name] = body
    return {k: renumber_labels(strip_padding(v)) for k, v in out.items()}


def strip_padding(body):
    """the s_nop padding behind a kernel is not its code.  Behind the LAST kernel of a code object it runs to the section's end and is
    followed by the next object's section header: a kernel that becomes or stops being the last one of its object would otherwise read
    DIFFERENT.  Counts and hashes are therefore not those of the profile files written before this function existed
    (profiles/r5_split_isa.txt, dispatch_refactor_isa.txt, host_common_refactor_isa.txt: e.g. plant_kernel 1346 there, 1089 now); verdicts
    within one file are unaffected, both columns of a file come from the same version of this script."""
    while body and (body[-1] == "s_nop 0" or body[-1].startswith("Disassembly of section")):
        body = body[:-1]
    return body


def renumber_labels(body):
    """the disassembler numbers the labels of a code object in sequence over its functions: a kernel's labels shift when a kernel
    in front of it is added or removed.  Number them per function, in order of first appearance."""
    ids = {}
    return [re.sub(r"\bL(\d+)\b", lambda m: "L%d" % ids.setdefault(m.group(1), len(ids)), t) for t in body]


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
same = True
for k in sorted(set(a) | set(b)):
    ha = hashlib.md5("\n".join(a.get(k, [])).encode()).hexdigest()[:12]
    hb = hashlib.md5("\n".join(b.get(k, [])).encode()).hexdigest()[:12]
    ok = ha == hb
    same &= ok
    verdict = "same" if ok else ("DIFFERENT" if k in a and k in b else "missing in " + (sys.argv[1] if k not in a else sys.argv[2]))
    print(f"{k[:70]:70s} {len(a.get(k, [])):7d} {ha}   {len(b.get(k, [])):7d} {hb}   {verdict}")
print("IDENTICAL device code" if same else "device code DIFFERS")
sys.exit(0 if same else 1)
