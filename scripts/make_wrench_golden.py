#!/usr/bin/env python3
"""Build tests/golden/wrench_tables.npz: the recorded disturbance tables the reference's applyBodyWrench() plays back in its
READ_WRENCH == 2 mode (bluerov2_dobmpc/src/bluerov2_dob.cpp:818-874), as ONE array for brov_plant_wrench_table_host.

Inputs (recorded data, one value per line, 496 lines each): bluerov2_dobmpc/config/forcex.txt, forcey.txt, forcez.txt, torquez.txt of
the reference tree.  Output: `table` [496][6] float64 = (fx, fy, fz, 0, 0, tz) per row, `sha256` = the digest of the four files'
bytes concatenated in that order (tests/test_wrench_restatement.py checks the fixture against it through `table_sha256`, the digest of
the array's own bytes, so that the check needs no reference tree).

    python scripts/make_wrench_golden.py [reference root, default /root/reference]
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("forcex.txt", "forcey.txt", "forcez.txt", "torquez.txt")
REFERENCE = "/root/reference"   # where scripts/make_golden.py reads the reference tree too


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else REFERENCE
    cfg = os.path.join(ref, "bluerov2_dobmpc", "config")
    raw = [open(os.path.join(cfg, f), "rb").read() for f in FILES]
    cols = [np.array([float(v) for v in r.split()], dtype=np.float64) for r in raw]
    rows = len(cols[0])
    assert all(len(c) == rows for c in cols), [len(c) for c in cols]
    table = np.zeros((rows, 6))
    table[:, 0], table[:, 1], table[:, 2], table[:, 5] = cols
    out = os.path.join(ROOT, "tests", "golden", "wrench_tables.npz")
    np.savez_compressed(out, table=table, sha256=np.array(hashlib.sha256(b"".join(raw)).hexdigest()),
                        table_sha256=np.array(hashlib.sha256(np.ascontiguousarray(table).tobytes()).hexdigest()),
                        files=np.array(FILES))
    print(f"{out}: table {table.shape}, |f|max = {np.abs(table).max():.3f}, inputs sha256 {hashlib.sha256(b''.join(raw)).hexdigest()}")


if __name__ == "__main__":
    main()
