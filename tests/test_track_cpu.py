"""Tracking statistics of closed loops (brov_track_*, brov_closed_loop_track) without a GPU: hand-computed answers of the numpy
restatement the kernels are held to, the C ABI's symbols, the record layout of the Python mirror, and the kernels' resource report."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from track_restatement import TrackRestatement, STATS_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BROV_TRACK_SYMBOLS = ["brov_track_default_params", "brov_track_last_error", "brov_track_create", "brov_track_destroy", "brov_track_batch",
                      "brov_track_reset", "brov_track_accumulate_host", "brov_track_accumulate_device", "brov_track_get_stats_host",
                      "brov_track_get_summary_host", "brov_track_last_seconds"]


def _hand_log():
    """2 instances, 3 ticks, a table of 3 rows, line1 = 1: tick 0 -> row 1, tick 1 -> row 2, tick 2 -> row 3, clamped to row 2"""
    ref = np.zeros((3, 16)); ref[:, 0] = [0, 1, 2]; ref[:, 5] = [0, 0.5, 1.0]
    x = np.zeros((3, 2, 12)); u = np.zeros((3, 2, 4)); st = np.zeros((3, 2), dtype=np.int32)
    # instance 0
    x[0, 0, [0, 1, 2, 5]] = [2, 2, 2, 2.5]; u[0, 0] = [1, 2, 3, 4]                  # e = (1, 2, 2): e2 = 9, yaw error 2
    x[1, 0, [0, 1, 2, 5]] = [7, np.nan, 7, 7]; u[1, 0] = [9, 9, 9, 9]; st[1, 0] = 3  # non-finite and failed
    x[2, 0, [0, 1, 2, 5]] = [5, 0, 0, 0.0]; u[2, 0] = [50, 0, 0, 0]                 # against row 2: e2 = 9 again (a tie), yaw error -1, at ubu
    # instance 1
    x[0, 1, [0, 1, 2, 5]] = [1, 3, 0, 0.5]; u[0, 1] = [-50, 1, 1, 1]                # e2 = 9 (the tie between instances), at lbu
    x[1, 1, [0, 1, 2, 5]] = [3, 0, 0, 4.0]                                          # e2 = 1, yaw error 3
    x[2, 1, [0, 1, 2, 5]] = [2, 0, 2, 1.0]; u[2, 1] = [1, 1, 1, 1]; st[2, 1] = 4    # e2 = 4, failed but finite: counted
    x[:, :, [3, 4, 6, 7, 8, 9, 10, 11]] = 123.0                                     # the other columns are not scored
    return x, u, st, ref


def test_restatement_against_hand_computed_answers():
    x, u, st, ref = _hand_log()
    r = TrackRestatement(2).accumulate(x, u, st, ref, line1=1)
    a, b = r.stats()
    assert (a["sum_pos2"], a["sum_yaw2"], a["max_pos2"], a["max_yaw"]) == (18.0, 5.0, 9.0, 2.0)
    assert list(a["sum_u2"]) == [2501.0, 4.0, 9.0, 16.0]          # the NaN tick's inputs (9, 9, 9, 9) are not in the sums
    assert (a["ticks"], a["failed"], a["saturated"], a["nonfinite"], a["first_failed"], a["worst_tick"]) == (2, 1, 1, 1, 1, 0)
    assert (b["sum_pos2"], b["sum_yaw2"], b["max_pos2"], b["max_yaw"]) == (14.0, 9.0, 9.0, 3.0)
    assert list(b["sum_u2"]) == [2501.0, 2.0, 2.0, 2.0]
    assert (b["ticks"], b["failed"], b["saturated"], b["nonfinite"], b["first_failed"], b["worst_tick"]) == (3, 1, 1, 0, 2, 0)
    assert not a["pad_"].any() and not b["pad_"].any()
    s = r.summary()
    assert s["rms_pos"] == math.sqrt(32.0 / 5.0) and s["rms_yaw"] == math.sqrt(14.0 / 5.0)
    assert (s["worst_max_pos2"], s["worst_instance"]) == (9.0, 0)                  # equal maxima: the lower index
    assert (s["ticks"], s["failed"], s["saturated"], s["nonfinite"], s["failed_instances"]) == (5, 2, 2, 1, 2)


def test_restatement_does_not_depend_on_the_cut_and_numbers_ticks_from_the_reset():
    x, u, st, ref = _hand_log()
    whole = TrackRestatement(2).accumulate(x, u, st, ref, 1).stats()
    cut = TrackRestatement(2)
    cut.accumulate(x[:1], u[:1], st[:1], ref, 1).accumulate(x[1:], u[1:], st[1:], ref, 2)
    assert cut.stats().tobytes() == whole.tobytes()
    cut.reset()
    cut.accumulate(x[2:], u[2:], st[2:], ref, 3)
    assert list(cut.stats()["first_failed"]) == [-1, 0] and list(cut.stats()["worst_tick"]) == [0, 0]


def test_restatement_infinite_input_no_status_and_empty_batch():
    x, u, _, ref = _hand_log()
    u[0, 1, 2] = -np.inf
    r = TrackRestatement(2).accumulate(x, u, None, ref, 1)
    a, b = r.stats()
    assert (a["failed"], a["first_failed"], b["failed"], b["first_failed"]) == (0, -1, 0, -1)
    assert (b["ticks"], b["nonfinite"], b["max_pos2"], b["worst_tick"], b["saturated"]) == (2, 1, 4.0, 2, 0)
    # no counted tick at all: zeros, worst instance -1 -- fresh, and after ticks that were all non-finite
    e = TrackRestatement(3)
    s = e.summary()
    assert (s["rms_pos"], s["rms_yaw"], s["worst_max_pos2"], s["worst_instance"], s["ticks"]) == (0.0, 0.0, 0.0, -1, 0)
    xn = np.full((2, 3, 12), np.nan)
    s = e.accumulate(xn, np.zeros((2, 3, 4)), None, ref, 0).summary()
    assert (s["rms_pos"], s["worst_max_pos2"], s["worst_instance"], s["ticks"], s["nonfinite"]) == (0.0, 0.0, -1, 0, 6)
    assert list(e.stats()["worst_tick"]) == [-1, -1, -1]
    # an instance without a counted tick cannot be the worst, even when every error is zero
    x0 = np.zeros((1, 3, 12)); x0[0, 0, 0] = np.nan
    s = TrackRestatement(3).accumulate(x0, np.zeros((1, 3, 4)), None, np.zeros((1, 16)), 5).summary()
    assert (s["worst_instance"], s["worst_max_pos2"], s["ticks"]) == (1, 0.0, 2)


def test_library_exports_every_track_symbol():
    import bluerov2_amd
    bluerov2_amd.build_library()
    lib = ctypes.CDLL(bluerov2_amd.library_path())
    missing = [n for n in BROV_TRACK_SYMBOLS + ["brov_closed_loop_track"] if not hasattr(lib, n)]
    assert not missing, missing
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bluerov2_nmpc.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(brov_track_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(BROV_TRACK_SYMBOLS)
    assert re.search(r"int brov_closed_loop_track\(brov_solver\* s, brov_ekf\* e\s*, brov_rls\* r\s*, int rls_mode, brov_track\* t,\s*"
                     r"int ticks, int line0, int ncols, double dt, int substeps, int chunk\);", txt)


def test_record_layout_and_default_bounds():
    import bluerov2_amd as ba
    d = ba.TRACK_STATS_DTYPE
    assert d.itemsize == 96 and d == STATS_DTYPE
    names = ("sum_pos2", "sum_yaw2", "max_pos2", "max_yaw", "sum_u2", "ticks", "failed", "saturated", "nonfinite", "first_failed",
             "worst_tick", "pad_")
    assert [d.fields[k][1] for k in names] == [0, 8, 16, 24, 32, 64, 68, 72, 76, 80, 84, 88]
    p = ba.TrackParams.default()
    o = ba.SolverOptions(20)
    assert list(p.lbu) == list(o.lbu) and list(p.ubu) == list(o.ubu) and ctypes.sizeof(p) == 64
    from bluerov2_amd.track import TrackSummary
    assert ctypes.sizeof(TrackSummary) == 64
    assert callable(ba.BatchSolver.closed_loop_track)
    for name in ("reset", "accumulate", "stats", "summary", "close"):
        assert callable(getattr(ba.BatchTrack, name))


def test_no_cpu_fallback():
    import torch
    import bluerov2_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(bluerov2_amd.NoDeviceError):
        bluerov2_amd.BatchTrack(4)


def test_track_kernels_use_no_scratch_and_the_makefile_gates_them():
    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "dev", "kernel_resources.sh"), "track_kernel.hip"], capture_output=True,
                         text=True, timeout=600).stdout
    rep = {}
    for ln in out.splitlines():
        m = re.match(r"Name: (\S+)", ln)
        if m:
            rep[m.group(1)] = {k: int(v) for k, v in re.findall(r"\|([A-Za-z ]+): (\d+)", ln)}
    kernels = ("track_accumulate_kernel", "track_reduce_kernel", "track_finish_kernel")
    names = {short: r for mangled, r in rep.items() for short in kernels if re.search(r"\d+%sE" % short, mangled)}
    assert set(names) == set(kernels), sorted(rep)
    for short, r in names.items():
        assert r["scratch"] == 0, (short, r)
    mk = open(os.path.join(ROOT, "bluerov2_amd", "csrc", "Makefile")).read()
    assert "track_kernel.hip" in mk.split("SRCS")[1].splitlines()[0]
    rule = mk[mk.index("$(OUTDIR)/obj/track_kernel.o:"):]
    rule = rule[:rule.index("\n\n")]
    assert "kernel-resource-usage" in rule and "ScratchSize" in rule and "track_accumulate_kernel" in rule and "rm -f $@" in rule
