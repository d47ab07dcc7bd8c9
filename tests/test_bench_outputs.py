"""bench.py's plain line and --dump-outputs: the plain run times --steps steps and prints the headline fields only (everything else is
behind --full); the outputs of its last timed step land as float64 .npy files, identical from run to run, within the size budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_is_the_default_and_full_is_an_option():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, "", 7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert (a.full, a.dump_outputs) == (True, "d")


def _fake_outputs(B, N, seed):
    rng = np.random.default_rng(seed)
    arrs = {f: rng.normal(size=(B,) + sh) for f, sh in (("u0", (4,)), ("cost", ()), ("kkt", ()), ("status", ()), ("qp_iter", ()),
                                                         ("thrust", (6,)), ("x", (N + 1, 12)), ("u", (N, 4)), ("pi", (N, 12)), ("lam", (N, 8)))}
    arrs["cost"] = np.arange(B, dtype=np.float64)   # the instance index: shows which instances a sample kept
    return arrs


def test_write_outputs_keeps_everything_within_the_budget(tmp_path):
    import bench
    arrs = _fake_outputs(64, 4, 1)
    bench.write_outputs(str(tmp_path), [("", arrs)])
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in arrs)
    for k, a in arrs.items():
        b = np.load(tmp_path / f"{k}.npy")
        assert b.dtype == np.float64 and np.array_equal(a, b)


def test_write_outputs_samples_the_same_instances_everywhere_when_over_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 400_000)
    outs = [("N10_", _fake_outputs(300, 10, 2)), ("N40_", _fake_outputs(300, 40, 3))]
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), outs)
    files = sorted(os.listdir(tmp_path / "a"))
    assert len(files) == 20 and sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 400_000
    for prefix, arrs in outs:
        keep = np.load(tmp_path / "a" / f"{prefix}cost.npy").astype(int)
        assert 0 < len(keep) < 300 and np.all(np.diff(keep) > 0)
        for k, a in arrs.items():
            b = np.load(tmp_path / "a" / f"{prefix}{k}.npy")
            assert b.dtype == np.float64 and np.array_equal(b, a[keep])
            assert np.array_equal(b, np.load(tmp_path / "b" / f"{prefix}{k}.npy"))   # a fixed sample


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs_are_reproducible(tmp_path):
    lines, dirs = [], []
    for run in range(2):
        d = tmp_path / f"out{run}"
        pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                             "--dump-outputs", str(d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        js = [ln for ln in pr.stdout.splitlines() if ln.startswith("{")]
        assert pr.returncode == 0 and len(js) == 1, (pr.returncode, pr.stdout[-2000:], pr.stderr[-2000:])
        lines.append(json.loads(js[0]))
        dirs.append(d)
    o = lines[0]
    assert o["unit"] == "solves/s" and o["higher_is_better"] is True and o["dtype"] == "f64" and o["steps"] == 3 and o["warmup"] == 1
    assert o["value"] > 0 and abs(o["value"] - 4096 / (o["ms_per_step"] * 1e-3)) < 1e-6 * o["value"]
    assert o["solver_status_nonzero"] == 0
    for k in ("roofline", "cpu_baseline", "forced_ipm", "configs", "batch1_tick"):    # --full only
        assert k not in o, k
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) and "u0.npy" in names and "x.npy" in names
    assert sum(os.path.getsize(dirs[0] / n) for n in names) <= 64 * 10**6
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype == np.float64 and a.shape[0] == 4096 and np.array_equal(a, b), n
    assert np.load(dirs[0] / "x.npy").shape == (4096, 21, 12) and np.all(np.load(dirs[0] / "status.npy") == 0)
