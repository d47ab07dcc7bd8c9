"""Host-side mirror of the batched tracking statistics (include/bluerov2_nmpc.h, brov_track_*): closed loops scored on the device
instead of logged.  ctypes over the HIP library -- no CPU path."""
import ctypes as C

import numpy as np

from .solver import _Handle, _arr, _bind, _dp, _load

# brov_track_stats, 96 bytes per instance
TRACK_STATS_DTYPE = np.dtype([("sum_pos2", "f8"), ("sum_yaw2", "f8"), ("max_pos2", "f8"), ("max_yaw", "f8"), ("sum_u2", "f8", (4,)),
                              ("ticks", "i4"), ("failed", "i4"), ("saturated", "i4"), ("nonfinite", "i4"), ("first_failed", "i4"),
                              ("worst_tick", "i4"), ("pad_", "i4", (2,))])
assert TRACK_STATS_DTYPE.itemsize == 96


class TrackParams(C.Structure):
    """brov_track_params: the input bounds `saturated` is judged by; TrackParams.default() = the bounds of brov_default_opts"""
    _fields_ = [("lbu", C.c_double * 4), ("ubu", C.c_double * 4)]

    @classmethod
    def default(cls):
        p = cls()
        _track_lib().brov_track_default_params(C.byref(p))
        return p


class TrackSummary(C.Structure):
    """brov_track_summary"""
    _fields_ = [("rms_pos", C.c_double), ("rms_yaw", C.c_double), ("worst_max_pos2", C.c_double), ("ticks", C.c_int64),
                ("failed", C.c_int64), ("saturated", C.c_int64), ("nonfinite", C.c_int64), ("worst_instance", C.c_int32),
                ("failed_instances", C.c_int32)]


def _protos(L):
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.brov_track_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(TrackParams)]
    _bind(L, {"brov_track_last_error": []}, C.c_char_p)
    _bind(L, {"brov_track_default_params": [C.POINTER(TrackParams)], "brov_track_destroy": [vp]}, None)
    _bind(L, {
        "brov_track_batch": [vp], "brov_track_reset": [vp],
        "brov_track_accumulate_host": [vp, dp, dp, ip, C.c_int, dp, C.c_int, C.c_int],
        "brov_track_accumulate_device": [vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp],
        "brov_track_get_stats_host": [vp, vp], "brov_track_get_summary_host": [vp, C.POINTER(TrackSummary)],
        "brov_track_last_seconds": [vp, dp],
        "brov_closed_loop_track": [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int],
    })


def _track_lib():
    return _load(_protos)


class BatchTrack(_Handle):
    """One tracking-statistics record per instance, resident on one GPU (brov_track).  Fed by accumulate() from logs or by
    BatchSolver.closed_loop_track(); stats() = the records, summary() = the whole batch."""
    _last_error, _destroy = "brov_track_last_error", "brov_track_destroy"

    def __init__(self, batch, params=None, device=0):
        L = _track_lib()
        self.B = int(batch)
        self.params = params if params is not None else TrackParams.default()
        self._create(L, "brov_track_create", int(device), self.B, C.byref(self.params))

    def reset(self):
        self._chk(self._L.brov_track_reset(self._h), "reset")

    def accumulate(self, x, u, status, ref, line1):
        """K ticks of host logs x [K, B, 12], u [K, B, 4], status [K, B] (None: all zero) against the table ref [rows, 16]: tick j against
        row min(line1 + j, rows - 1)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        K = x.shape[0] if x.ndim == 3 else 0
        x = _arr(x, (K, self.B, 12)); u = _arr(u, (K, self.B, 4))
        ref = np.ascontiguousarray(ref, dtype=np.float64)
        if ref.ndim != 2 or ref.shape[1] != 16:
            raise ValueError(f"expected a table [rows, 16], got {ref.shape}")
        sp = None
        if status is not None:
            status = _arr(status, (K, self.B), np.int32)
            sp = status.ctypes.data_as(C.POINTER(C.c_int32))
        self._chk(self._L.brov_track_accumulate_host(self._h, _dp(x), _dp(u), sp, K, _dp(ref), ref.shape[0], int(line1)), "accumulate")

    def accumulate_device(self, x_ptr, u_ptr, status_ptr, K, ref_ptr, rows, line1, stream=0):
        """the same through device pointers (status_ptr 0 / None: all zero); enqueued on `stream`, no host wait"""
        self._chk(self._L.brov_track_accumulate_device(self._h, C.c_void_p(x_ptr), C.c_void_p(u_ptr), C.c_void_p(status_ptr or None), int(K),
                                                       C.c_void_p(ref_ptr), int(rows), int(line1), C.c_void_p(stream)), "accumulate_device")

    def stats(self):
        """the records, a structured array [B] of TRACK_STATS_DTYPE"""
        out = np.empty(self.B, dtype=TRACK_STATS_DTYPE)
        self._chk(self._L.brov_track_get_stats_host(self._h, out.ctypes.data_as(C.c_void_p)), "stats")
        return out

    def summary(self):
        """dict of the batch summary (brov_track_summary) plus worst_max_pos = sqrt(worst_max_pos2)"""
        s = TrackSummary()
        self._chk(self._L.brov_track_get_summary_host(self._h, C.byref(s)), "summary")
        d = {k: getattr(s, k) for k, _ in TrackSummary._fields_}
        d["worst_max_pos"] = float(np.sqrt(s.worst_max_pos2))
        return d

    def summary_bytes(self):
        """the raw 64 bytes of brov_track_summary (two calls return the same bytes)"""
        s = TrackSummary()
        self._chk(self._L.brov_track_get_summary_host(self._h, C.byref(s)), "summary")
        return bytes(s)

    def last_seconds(self):
        s = C.c_double()
        self._chk(self._L.brov_track_last_seconds(self._h, C.byref(s)), "last_seconds")
        return s.value
