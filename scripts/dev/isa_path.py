#!/usr/bin/env python3
"""isa_path.py <object or library> [kernel name substring] [N] -- the EARLY-EXIT path of one one-wave fused kernel, counted in issue slots.

A SIMD is visited once every four cycles, so with ONE resident wave every instruction -- vector, scalar, LDS, s_waitcnt, s_nop, branch -- costs a
four-cycle slot; an FP64 MFMA holds the SIMD for 64.  The model is therefore  cycles = 4 x instructions + 60 x MFMAs.

The path is: head (staging, cost gradients, state integration) -> general columns loop -> closed-form columns loop -> straight line (columns'
tail, setup_inst, operand offset tables, bwd_init) -> factor loop (step 0) -> forward loop -> bound check -> adjoint loop with commit -> commit
loops.  The five loops are found by their signatures (the same loops scripts/dev/isa_loops.py lists; profiles/r6_fused_phase_isa.txt names
them); the straight-line sections that are contiguous in the code (head, between the column loops, between the column loops and the factor loop)
are counted as address ranges -- an upper bound where a guarded block (dump_lin, a debug hook) is jumped over.  What lies behind the factor loop
is reached by jumps over the QP loop's code and is NOT walked: its dynamic count is the measured total (scripts/dev/issue_slot_counters.py) minus
the rows below.  Trip counts: every sweep loop holds three stages per trip (N / 3 trips; the remainder stages run in copies of the body outside
the loop and are modelled as a fraction of a trip), the general-columns loop runs `--general` trips (1 at N = 20) and the closed-form loop
`--closed` (2 at N = 20).

`loops(path, kernel)` returns {name: (start, end, Counter of classes)} for tests/test_fused_issue_budget.py."""
import argparse
import collections
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import check_exec_restore as C

CL = [("mfma", r"^v_mfma"), ("f64 dpp", r"^v_.*_f64_dpp"), ("f64", r"^v_(fma|mul|add|fmac|fmamk|fmaak|max|min|rcp|rsq|ldexp)_f64"),
      ("cmp", r"^v_cmp"), ("cndmask", r"^v_cndmask"), ("readlane", r"^v_read"), ("writelane", r"^v_writelane"), ("accvgpr", r"^v_accvgpr"),
      ("mov/bit", r"^v_(mov|bfi|and|or|xor|not|lshl|lshr|ashr|perm|swap|bfe)"),
      ("mul32", r"^v_(mul_lo|mul_hi|mad_u64)"), ("int", r"^v_(add|sub|mul|mad|lshl_add|add_lshl|min|max)_(u|i|co|nc)"), ("valu other", r"^v_"),
      ("lds", r"^ds_"), ("vmem", r"^(global|flat|buffer|scratch)_"), ("smem", r"^s_(load|buffer_load|memtime|memrealtime)"),
      ("wait/nop", r"^s_(waitcnt|nop|barrier|sleep|setprio)"), ("branch", r"^s_(cbranch|branch|endpgm)"), ("salu", r"^s_")]
VALU = ("f64 dpp", "f64", "cmp", "cndmask", "readlane", "writelane", "accvgpr", "mov/bit", "mul32", "int", "valu other")
LOOPS = ("general columns", "closed-form columns", "factor (step 0)", "forward", "adjoint + commit")


def cls(m):
    for n, p in CL:
        if re.match(p, m):
            return n
    return "?"


def instructions(path, want):
    """(mnemonic, branch target index or None) per instruction of the first kernel whose name contains `want`"""
    C.OBJDUMP = C.OBJDUMP or C.find_objdump()
    name, lines = None, []
    for ln in C.listing(path):
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", ln)
        if m and not m.group(1).startswith("L"):
            if lines:
                break
            name = m.group(1)
        if name and want in name:
            lines.append(ln)
    lab, toks = {}, []
    for l in lines:
        m = re.match(r"^[0-9a-f]+ <(L\d+)>:", l)
        if m:
            lab[m.group(1)] = len(toks)
            continue
        t = l.split("//")[0].split()
        if t and not t[0].endswith(":") and not re.match(r"^[0-9a-f]+$", t[0]):
            toks.append(t)
    return name, [(t[0], lab.get(t[-1]) if t[0].startswith(("s_cbranch", "s_branch")) else None) for t in toks]


def all_loops(ins, minlen=100):
    """(start, end, classes) per loop header: from the header to its LAST backward branch (a three-stage body whose guards the compiler
    turned into early continues has several)"""
    last = {}
    for i, (m, tgt) in enumerate(ins):
        if tgt is not None and tgt < i:
            last[tgt] = i
    return sorted((t, i + 1, collections.Counter(cls(x[0]) for x in ins[t:i + 1])) for t, i in last.items() if i + 1 - t >= minlen)


def loops(path, want="16rti_fused_kernelENS"):
    """the five loops of the early-exit path by signature, in path order"""
    name, ins = instructions(path, want)
    ls = all_loops(ins)
    nodpp = lambda h: h["mfma"] == 0 and h["f64 dpp"] == 0
    gen = next(l for l in ls if nodpp(l[2]) and l[2]["f64"] >= 600)
    clo = next(l for l in ls if l[0] >= gen[1] and nodpp(l[2]) and l[2]["f64"] >= 200)
    fac = next(l for l in ls if l[0] >= clo[1] and l[2]["mfma"] >= 27 and l[2]["mfma"] % 9 == 0)   # whole stages: 9 MFMAs each
    # (the sweep runs as two chunks around the checkpoint of the partial refactorisation, which the compiler makes a loop of two trips around
    # the stage loop: the stage loop is the innermost loop that holds all of its MFMAs)
    fac = min((l for l in ls if fac[0] <= l[0] and l[1] <= fac[1] and l[2]["mfma"] == fac[2]["mfma"]), key=lambda l: l[1] - l[0])
    fwd = next(l for l in ls if l[0] >= fac[1] and l[2]["f64 dpp"] >= 16 and l[2]["mfma"] == 0 and l[1] - l[0] < 400)
    adj = [l for l in ls if l[0] >= fwd[1] and nodpp(l[2]) and l[2]["f64"] >= 20 and l[2]["lds"] >= 20 and l[2]["vmem"] == 0 and l[1] - l[0] < 400][-1]
    return name, ins, collections.OrderedDict(zip(LOOPS, (gen, clo, fac, fwd, adj)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path"); ap.add_argument("kernel", nargs="?", default="16rti_fused_kernelENS"); ap.add_argument("N", nargs="?", type=int, default=20)
    ap.add_argument("--general", type=float, default=1.0); ap.add_argument("--closed", type=float, default=2.0)
    a = ap.parse_args()
    name, ins, L = loops(a.path, a.kernel)
    gen, clo, fac = L[LOOPS[0]], L[LOOPS[1]], L[LOOPS[2]]
    # stages per trip of a sweep loop: the compiler rotates the three-stage bodies (a loop may hold two of them, the third outside): counted
    # by the stage's own arithmetic -- 9 MFMAs per factor stage, 16 DPP multiply-adds per forward stage, 10 FP64 operations per adjoint stage
    per = (fac[2]["mfma"] / 9.0, L[LOOPS[3]][2]["f64 dpp"] / 16.0, L[LOOPS[4]][2]["f64"] / 10.0)
    trips = dict(zip(LOOPS, (a.general, a.closed, a.N / per[0], a.N / per[1], a.N / per[2])))
    rows = [("head", 0, gen[0], 1.0), (LOOPS[0], *gen[:2], trips[LOOPS[0]]), ("between the column loops", gen[1], clo[0], 1.0),
            (LOOPS[1], *clo[:2], trips[LOOPS[1]]), ("columns' tail .. bwd_init", clo[1], fac[0], 1.0)] + \
           [(n, *L[n][:2], trips[n]) for n in LOOPS[2:]]
    order = [c for c, _ in CL]
    print(f"{name}: {len(ins)} instructions; early-exit path at N = {a.N} (static counts x trips; cycles = 4 x instructions + 60 x MFMA)")
    print(f"  {'section':26s} {'range':>15s} {'instr':>6s} {'trips':>6s} {'dynamic':>8s} {'VALU':>6s} {'MFMA':>5s} {'cycles':>8s} | classes (static)")
    tot = collections.Counter(); tn = tc = 0.0
    for nm, s, e, t in rows:
        h = collections.Counter(cls(x[0]) for x in ins[s:e])
        n = sum(h.values()); valu = sum(h[c] for c in VALU)
        cyc = t * (4 * n + 60 * h["mfma"])
        tn += t * n; tc += cyc
        for c, v in h.items():
            tot[c] += t * v
        print(f"  {nm:26s} {s:6d} ..{e:6d} {n:6d} {t:6.2f} {t * n:8.0f} {t * valu:6.0f} {t * h['mfma']:5.0f} {cyc:8.0f} | " +
              " ".join(f"{c}={h[c]}" for c in order if h[c]))
    print(f"  {'sum':26s} {'':15s} {'':6s} {'':6s} {tn:8.0f} {sum(tot[c] for c in VALU):6.0f} {tot['mfma']:5.0f} {tc:8.0f} | " +
          " ".join(f"{c}={tot[c]:.0f}" for c in order if tot[c]))
    print("  (not walked: factor epilogue -> forward prologue, bound check, early-exit tail, commit loops: measured total minus the sum)")


if __name__ == "__main__":
    main()
