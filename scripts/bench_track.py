#!/usr/bin/env python3
"""Cost of scoring a closed loop on the device instead of logging it (brov_track_*, brov_closed_loop_track).

At B = 4096 and 16 384, N = 20, for the same `--ticks` ticks of the circle from the same start:
1. seconds of closed_loop_track (chunks of `--chunk` ticks) beside closed_loop(log=False) -- the tracking overhead: same build, same ticks,
   no logs on either side -- and beside closed_loop(log=True) -- the saving: device logs for the whole run, copied to the host;
2. seconds of ONE accumulate call over a chunk of device logs (brov_track_last_seconds: HIP events around the kernel);
3. peak device bytes of the logs: one chunk against the whole run.

Median of `--repeats` runs after one warm-up run each.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG_BYTES_PER_INSTANCE_TICK = 12 * 8 + 4 * 8 + 4      # state after the tick, applied input, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="4096,16384")
    ap.add_argument("--ticks", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import bluerov2_amd as ba
    from bench import synthetic_inputs
    N, rows = 20, []
    for B in [int(b) for b in a.batch.split(",")]:
        x0, circ = synthetic_inputs(B, seed=3)
        pp = np.tile(ba.P_NOMINAL, (B, 1))
        s = ba.BatchSolver(B, ba.SolverOptions(N, 0.05))
        s.set_params(ba.P_NOMINAL); s.set_plant_params(pp); s.set_trajectory(circ)
        t = ba.BatchTrack(B)
        chunk = a.chunk if a.chunk > 0 else 64

        def run(which):
            s.set_x0(x0); s.init_iterate_default(); t.reset()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            if which == "track":
                s.closed_loop_track(t, a.ticks, chunk=a.chunk)
            else:
                s.closed_loop(a.ticks, log=(which == "log"))
            return time.perf_counter() - t0
        row = {"batch": B}
        for which in ("nolog", "track", "log"):
            run(which)
            dts = [run(which) for _ in range(a.repeats)]
            row[which] = {"seconds_median": float(np.median(dts)), "seconds_min": float(np.min(dts)), "seconds_max": float(np.max(dts)),
                          "instance_ticks_per_s": B * a.ticks / float(np.median(dts))}
        run("track")
        row["accumulate_seconds_per_chunk"] = t.last_seconds()            # the last chunk of the run
        row["accumulate_ticks_in_that_chunk"] = a.ticks - ((a.ticks - 1) // chunk) * chunk
        row["summary"] = t.summary()
        row["track_overhead_vs_nolog"] = row["track"]["seconds_median"] / row["nolog"]["seconds_median"] - 1.0
        row["track_saving_vs_log"] = 1.0 - row["track"]["seconds_median"] / row["log"]["seconds_median"]
        row["log_bytes_one_chunk"] = min(chunk, a.ticks) * B * LOG_BYTES_PER_INSTANCE_TICK
        row["log_bytes_whole_run"] = (a.ticks * LOG_BYTES_PER_INSTANCE_TICK + 12 * 8) * B
        rows.append(row)
        t.close(); s.close()
    print(json.dumps({"metric": "closed loop scored on the device against the unlogged and the logged loop, seconds per run", "N": N,
                      "ticks": a.ticks, "chunk": a.chunk, "repeats": a.repeats, "rows": rows}))


if __name__ == "__main__":
    main()
