"""The builder of the range stage's mesh hierarchy (bluerov2_amd/csrc/mesh_bvh.hpp) on the host alone: tests/mesh_bvh_main.cpp, a program
with its own main, compiled with -fsanitize=address,undefined and run directly -- no Python in the process, no preload.  Per case and leaf
size 1 ... 8: every triangle in exactly one leaf, every node box around its subtree and the pad, skip links strictly increasing and ending at
the node count, depth <= ceil(log2 T) + 1, and a forward walk that equals brute force on 200 rays."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("fixture", "icosphere", "one", "leaf_plus_one", "identical")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    from bluerov2_amd.mesh import icosphere
    tmp = tmp_path_factory.mktemp("mesh_bvh")
    exe = str(tmp / "mesh_bvh_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", f"-I{ROOT}/bluerov2_amd/csrc", os.path.join(ROOT, "tests", "mesh_bvh_main.cpp"), "-o", exe],
                   check=True, timeout=600)
    rng = np.random.default_rng(3)
    one = rng.uniform(-1, 1, (1, 3, 3))
    meshes = {"fixture": np.load(os.path.join(ROOT, "tests", "golden", "bridge2_piers.npz"))["tri"], "icosphere": icosphere(3),
              "one": one, "identical": np.repeat(one, 64, axis=0)}
    files = []
    for name, tri in meshes.items():
        files.append(str(tmp / name))
        np.ascontiguousarray(tri, dtype=np.float64).tofile(files[-1])
    for leaf in range(1, 9):                                  # T = leaf + 1: the smallest mesh that has to split
        files.append(str(tmp / f"leaf_plus_one{leaf}"))
        rng.uniform(-1, 1, (leaf + 1, 3, 3)).tofile(files[-1])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600, env=env)
    print(out.stdout[-6000:], out.stderr[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    got = {}
    for ln in out.stdout.splitlines():
        m = re.match(r"(\S+) leaf (\d) => (.*)", ln)
        if m:
            got[(os.path.basename(m.group(1)), int(m.group(2)))] = m.group(3)
    return got


@pytest.mark.parametrize("leaf", range(1, 9))
@pytest.mark.parametrize("case", CASES)
def test_structure(lines, case, leaf):
    name = f"leaf_plus_one{leaf}" if case == "leaf_plus_one" else case
    assert lines[(name, leaf)].startswith("ok "), lines[(name, leaf)]
    f = dict(zip(*[iter(lines[(name, leaf)].split()[1:])] * 2))
    if case == "leaf_plus_one":
        assert (int(f["nodes"]), int(f["leaves"]), int(f["depth"])) == (3, 2, 1)
    if case == "one":
        assert (int(f["nodes"]), int(f["leaves"]), int(f["depth"])) == (1, 1, 0)


def test_the_icosphere_has_the_expected_shape_and_the_walk_is_no_brute_force(lines):
    f = dict(zip(*[iter(lines[("icosphere", 4)].split()[1:])] * 2))
    assert (int(f["nodes"]), int(f["depth"])) == (1023, 9), f           # 1280 halves nine times to 2 and 3
    assert float(f["tri_tests"]) <= 1280 / 16, f
