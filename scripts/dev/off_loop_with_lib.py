#!/usr/bin/env python3
"""dev: `scripts/bench_clearance.py --only off` against ANOTHER build of the library, e.g. the one scripts/dev/build_head_lib.sh makes of the
commit before the clearance term, which has no brov_clearance_* symbols: the prototypes a library lacks are skipped (the off loop calls
none of them).  A fresh process per library; alternate the two for a side-by-side:
    python scripts/dev/off_loop_with_lib.py bluerov2_amd/lib/libbluerov2_nmpc.so
    python scripts/dev/off_loop_with_lib.py bluerov2_amd/lib/libbluerov2_nmpc_head.so"""
import ctypes as C
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import bluerov2_amd.fleet as F      # noqa: E402
import bluerov2_amd.solver as S     # noqa: E402

S._LIB = os.path.abspath(sys.argv[1])
_bind_all = S._bind


def _bind_present(L, table, restype=C.c_int):
    _bind_all(L, {k: v for k, v in table.items() if hasattr(L, k)}, restype)


S._bind = F._bind = _bind_present
sys.argv = ["bench_clearance.py", "--only", "off"] + sys.argv[2:]
runpy.run_path(os.path.join(ROOT, "scripts", "bench_clearance.py"), run_name="__main__")
