"""Host-side mirror of include/bluerov2_nmpc_inspect.h (ctypes): the structures of the range stage (brov_range_*) and of the inspection
controller (brov_inspect_*), their defaults, the records of the controller's state and statistics, and the pier of the reference's bridge
demo.  The calls themselves are methods of BatchSolver (solver.py): set_range_scene, set_range, range_eval, set_inspect, inspect_eval,
inspect_step, closed_loop_inspect, inspect_stats."""
import ctypes as C
import math

import numpy as np

RANGE_MAX_BOXES = 8                          # BROV_RANGE_MAX_BOXES
INSPECT_SHARED_PID, INSPECT_FLOAT_YAW = 1, 2   # BROV_INSPECT_*


class RangeParams(C.Structure):
    """brov_range_params: the depth camera's focal length and principal-point offset in pixels, its mount in the body frame, the clip
    distances, the noise seed and the side of the region of interest"""
    _fields_ = [("f", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("mount", C.c_double * 3), ("near", C.c_double), ("far", C.c_double),
                ("seed", C.c_uint64), ("roi", C.c_int32), ("reserved_", C.c_int32)]


class InspectParams(C.Structure):
    """brov_inspect_params: the VisualController's constants (include/bluerov2_nmpc_inspect.h names each)"""
    _fields_ = [(n, C.c_double) for n in ("dt", "safety_dis", "buffer", "sway", "sway_slow", "surge_search", "z0", "yaw0", "dz_round", "lost",
                                          "yaw_tol", "yaw_home_tol", "z_tol", "height_tol", "t_hold", "z_goal")] + \
               [("gains", C.c_double * 9), ("flags", C.c_int32), ("reserved_", C.c_int32)]


INSPECT_STATE_DTYPE = np.dtype([("integral", "f8", (3,)), ("prev_error", "f8", (3,)), ("yaw_sum", "f8"), ("pre_yaw", "f8"), ("ref_x", "f8"),
                                ("ref_z", "f8"), ("ref_yaw", "f8"), ("started", "i4"), ("turn", "i4"), ("completed_turn", "i4"),
                                ("completed_round", "i4"), ("get_height", "i4"), ("completed_mission", "i4"), ("cycle_counter", "i4"),
                                ("status", "i4"), ("k", "i8")])
INSPECT_STATS_DTYPE = np.dtype([("ticks", "i4", (6,)), ("rounds", "i4"), ("failed", "i4"), ("first_done", "i4"), ("reserved_", "i4"),
                                ("standoff_sq", "f8"), ("min_range", "f8")])
assert INSPECT_STATE_DTYPE.itemsize == 128 and INSPECT_STATS_DTYPE.itemsize == 56

# the pier of bluerov2_path/config/traj/bridge_vision.py in x, y; z over the water column
PIER_LO = (17.74002, 5.259887, -100.0)
PIER_HI = (21.34002, 8.97006, 10.0)
# the bridge demo's launch pose: x, y, z, yaw
START_POSE = (17.97842, 3.259887, -34.5, 0.5 * math.pi)


def range_focal(width, hfov):
    """focal length in pixels of a pinhole camera `width` pixels wide over the horizontal field of view `hfov` (rad): brov_range_focal"""
    return width / (2.0 * math.tan(hfov / 2.0))


def default_range_params():
    """brov_range_default_params: the depth sensor of the reference's camera (1280 pixels over 85.2 degrees), roi 40, clip 0.1 ... 100"""
    p = RangeParams()
    p.f = range_focal(1280.0, 85.2 * math.pi / 180.0)
    p.near, p.far, p.roi = 0.1, 100.0, 40
    return p


def default_inspect_params():
    """brov_inspect_default_params: the node's values, both of its quirks on"""
    p = InspectParams()
    p.dt, p.safety_dis, p.buffer, p.sway, p.sway_slow, p.surge_search, p.z0, p.yaw0 = 0.05, 1.79, 0.5, -4.0, -2.0, 1.0, -34.5, 0.5 * math.pi
    p.dz_round = p.safety_dis * math.tan(32 * math.pi / 180) * 2
    p.lost, p.yaw_tol, p.yaw_home_tol, p.z_tol, p.height_tol, p.t_hold = 0.1, 0.1, 0.2, 0.25, 0.1, 1.0
    p.z_goal = p.z0 + p.dz_round
    p.gains[:] = [5, 0, 0, 5, 0, 0, 7, 0.08, 0]
    p.flags = INSPECT_SHARED_PID | INSPECT_FLOAT_YAW
    return p


def initial_state(par, batch):
    """[batch] records of INSPECT_STATE_DTYPE: the state of the node's constructor under `par` (what brov_inspect_reset uploads)"""
    s = np.zeros(batch, dtype=INSPECT_STATE_DTYPE)
    y = float(np.float32(par.yaw0)) if par.flags & INSPECT_FLOAT_YAW else par.yaw0
    s["yaw_sum"], s["pre_yaw"], s["ref_x"], s["ref_z"], s["ref_yaw"] = y, y, par.safety_dis, par.z0, par.yaw0
    s["completed_turn"], s["get_height"] = 1, 1
    return s


def initial_stats(batch):
    t = np.zeros(batch, dtype=INSPECT_STATS_DTYPE)
    t["first_done"] = -1
    return t


def protos(bind, L):
    """the prototypes of the two families, declared through solver.py's `_bind`"""
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    bind(L, {
        "brov_range_set_scene_host": [vp, C.c_int32, dp, dp], "brov_range_set_host": [vp, C.POINTER(RangeParams), dp],
        "brov_range_eval_host": [vp, C.c_int64, dp, dp, ip, dp, dp], "brov_range_last_seconds": [vp, dp],
        "brov_inspect_set_host": [vp, C.POINTER(InspectParams)], "brov_inspect_off": [vp], "brov_inspect_enabled": [vp], "brov_inspect_reset": [vp],
        "brov_inspect_eval_host": [vp, vp, dp, dp, dp, vp, vp, vp], "brov_inspect_get_state_host": [vp, vp, dp],
        "brov_inspect_get_stats_host": [vp, vp], "brov_inspect_reset_stats": [vp], "brov_inspect_last_seconds": [vp, dp],
        "brov_inspect_step": [vp, vp], "brov_closed_loop_inspect": [vp, C.c_int, C.c_double, C.c_int, dp, dp, ip, dp],
    })
    bind(L, {"brov_range_default_params": [C.POINTER(RangeParams)], "brov_inspect_default_params": [C.POINTER(InspectParams)]}, None)
    bind(L, {"brov_range_focal": [C.c_double, C.c_double]}, C.c_double)
