"""numpy restatement of the tracking statistics (include/bluerov2_nmpc.h, brov_track_stats / brov_track_summary), the yardstick of
bluerov2_amd/csrc/track_kernel.hip.  It is the specification: the record is accumulated sequentially in tick order, in plain IEEE
arithmetic and in the order written here ((dx^2 + dy^2) + dz^2, no fused multiply-add: numpy rounds every operation), the summary is
reduced with plain sum / argmax."""
import numpy as np

STATS_DTYPE = np.dtype([("sum_pos2", "f8"), ("sum_yaw2", "f8"), ("max_pos2", "f8"), ("max_yaw", "f8"), ("sum_u2", "f8", (4,)),
                        ("ticks", "i4"), ("failed", "i4"), ("saturated", "i4"), ("nonfinite", "i4"), ("first_failed", "i4"),
                        ("worst_tick", "i4"), ("pad_", "i4", (2,))])


class TrackRestatement:
    def __init__(self, B, lbu=-50.0, ubu=50.0):
        self.B = int(B)
        self.lbu = np.broadcast_to(np.asarray(lbu, dtype=np.float64), (4,)).copy()
        self.ubu = np.broadcast_to(np.asarray(ubu, dtype=np.float64), (4,)).copy()
        self.reset()

    def reset(self):
        self.rec = np.zeros(self.B, dtype=STATS_DTYPE)
        self.rec["first_failed"] = -1
        self.rec["worst_tick"] = -1

    def accumulate(self, x, u, status, ref, line1):
        """x [K, B, 12], u [K, B, 4], status [K, B] or None, ref [rows, 16]; tick j against row min(line1 + j, rows - 1) (below 0: row 0)"""
        x, u, ref = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        K, rows, r = x.shape[0], ref.shape[0], self.rec
        for j in range(K):
            yr = ref[min(max(line1 + j, 0), rows - 1)]
            st = np.zeros(self.B, dtype=np.int32) if status is None else np.asarray(status[j])
            tick = r["ticks"] + r["nonfinite"]                   # numbered from the last reset
            bad = st != 0
            r["failed"] += bad
            first = bad & (r["first_failed"] < 0)
            r["first_failed"][first] = tick[first]
            pose = x[j][:, [0, 1, 2, 5]]
            fin = np.isfinite(pose).all(axis=1) & np.isfinite(u[j]).all(axis=1)
            r["nonfinite"] += ~fin
            with np.errstate(invalid="ignore", over="ignore"):
                dx, dy, dz, dpsi = pose[:, 0] - yr[0], pose[:, 1] - yr[1], pose[:, 2] - yr[2], pose[:, 3] - yr[5]
                e2 = (dx * dx + dy * dy) + dz * dz
                yaw2, ay, u2 = dpsi * dpsi, np.abs(dpsi), u[j] * u[j]
                sat = ((u[j] <= self.lbu) | (u[j] >= self.ubu)).any(axis=1)
                new_max = fin & ((r["ticks"] == 0) | (e2 > r["max_pos2"]))
                new_yaw = fin & (ay > r["max_yaw"])
            r["sum_pos2"][fin] = r["sum_pos2"][fin] + e2[fin]
            r["sum_yaw2"][fin] = r["sum_yaw2"][fin] + yaw2[fin]
            r["sum_u2"][fin] = r["sum_u2"][fin] + u2[fin]
            r["max_pos2"][new_max] = e2[new_max]
            r["worst_tick"][new_max] = tick[new_max]
            r["max_yaw"][new_yaw] = ay[new_yaw]
            r["saturated"] += fin & sat
            r["ticks"] += fin
        return self

    def stats(self):
        return self.rec.copy()

    def summary(self):
        r = self.rec
        live = r["ticks"] > 0
        out = dict(rms_pos=0.0, rms_yaw=0.0, worst_max_pos2=0.0, worst_instance=-1,
                   ticks=int(r["ticks"].astype(np.int64).sum()), failed=int(r["failed"].astype(np.int64).sum()),
                   saturated=int(r["saturated"].astype(np.int64).sum()), nonfinite=int(r["nonfinite"].astype(np.int64).sum()),
                   failed_instances=int((r["failed"] > 0).sum()))
        if live.any():
            idx = np.nonzero(live)[0]
            out["rms_pos"] = float(np.sqrt(r["sum_pos2"][live].sum() / out["ticks"]))
            out["rms_yaw"] = float(np.sqrt(r["sum_yaw2"][live].sum() / out["ticks"]))
            w = int(idx[np.argmax(r["max_pos2"][live])])         # argmax: the first, i.e. the lowest index on ties
            out["worst_instance"], out["worst_max_pos2"] = w, float(r["max_pos2"][w])
        return out
