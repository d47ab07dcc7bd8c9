"""Host-side mirror of include/bluerov2_nmpc.h (ctypes).  Names and argument meaning follow the reference call sites:

    reference (C++ ROS node, per 50 ms tick)                             here (B instances at once)
    ocp_nlp_constraints_model_set(..,0,"lbx"/"ubx",x0)                   BatchSolver.set_x0(x0[B,12])
    bluerov2_acados_update_params(capsule,i,p,16)  for i in 0..N         BatchSolver.set_params(p[B,16] | p[B,N+1,16])
    ocp_nlp_cost_model_set(..,i,"yref",yref[i])    for i in 0..N         BatchSolver.set_yref(yref[N+1,16] | [B,N+1,16])
    bluerov2_acados_solve(capsule)                                       BatchSolver.solve()
    ocp_nlp_out_get(..,0,"u",u0) / status / inf_norm_res                 BatchSolver.results() -> u0, cost, kkt, status
(/root/reference/bluerov2_dobmpc/src/bluerov2_dob.cpp:306-388, src/ctrller/mpc.cpp:40-197).
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import inspect as _inspect
from . import mesh as _mesh
from .mesh import MeshInfo, load_stl, MESH_MAX_TRIANGLES  # noqa: F401
from .inspect import (RangeParams, InspectParams, INSPECT_STATE_DTYPE, INSPECT_STATS_DTYPE, INSPECT_SHARED_PID,  # noqa: F401
                      INSPECT_FLOAT_YAW, RANGE_MAX_BOXES)

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(HERE, "lib", "libbluerov2_nmpc.so")
NX, NU, NP, NY = 12, 4, 16, 16
MAX_N = 256      # BROV_MAX_N (streaming pair)
MAX_N_LDS = 128  # BROV_MAX_N_LDS (LDS-resident kernels)
PATH_AUTO, PATH_STREAMING, PATH_FUSED, PATH_WINDOWED = 0, 1, 2, 3
WRENCH_OFF, WRENCH_CONSTANT, WRENCH_PERIODIC, WRENCH_TABLE = 0, 1, 2, 3   # BROV_WRENCH_*
CURRENT_OFF, CURRENT_CONSTANT, CURRENT_TABLE, CURRENT_GAUSS_MARKOV = 0, 1, 2, 3   # BROV_CURRENT_*
CORIOLIS_RIGID, CORIOLIS_ADDED = 1, 2   # BROV_CORIOLIS_*: a bit mask

# nominal hydrodynamic parameters the nodes pass every tick (bluerov2_dob.cpp:340-353); p[0:4] = disturbance
P_NOMINAL = np.array([0, 0, 0, 0, 1.7182, 0, 5.468, 0.4006, -11.7391, -20, -31.8678, -5, -18.18, -21.66, -36.99, -1.55])
ROTOR_CONSTANT = 0.026546960744430276

RESULT_DTYPE = np.dtype([("u0", "f8", (4,)), ("cost", "f8"), ("kkt", "f8"), ("status", "i4"), ("qp_iter", "i4"),
                         ("thrust", "f8", (6,))])
assert RESULT_DTYPE.itemsize == 104
ON_FAILURE_KEEP, ON_FAILURE_RESTART = 0, 1


class NoDeviceError(RuntimeError):
    pass


class ImuParams(C.Structure):
    """brov_imu_params: the IMU/GPS stage's step h, gravity, the GPS divider, BROV_IMU_* flags and the noise seed"""
    _fields_ = [("h", C.c_double), ("g", C.c_double), ("gps_every", C.c_int32), ("flags", C.c_int32), ("seed", C.c_uint64)]


IMU_GPSV_ELAPSED = 1


class CurveParams(C.Structure):
    """brov_curve_params of include/bluerov2_nmpc_curve.h"""
    _fields_ = [("kind", C.c_int32), ("pre", C.c_int32), ("quantum", C.c_double), ("k", C.c_double), ("kl", C.c_double), ("kr", C.c_double),
                ("dl", C.c_double), ("dr", C.c_double), ("pre_poly", C.c_double * 5), ("observer_applied", C.c_int32), ("reserved_", C.c_int32)]

    @classmethod
    def default(cls):
        p = cls()
        _load().brov_curve_default_params(C.byref(p))
        return p


CURVE_LINEAR, CURVE_BASIC, CURVE_DEADZONE, CURVE_TABLE = 0, 1, 2, 3
CURVE_PRE_NONE, CURVE_PRE_POLY, CURVE_PRE_TABLE = 0, 1, 2
CURVE_PART_COMMAND, CURVE_PART_THRUST, CURVE_PART_BOTH = 1, 2, 3
CURVE_WHICH_CURVE, CURVE_WHICH_PRE = 0, 1
CURVE_MAX_KNOTS = 256
_CURVE_KINDS = {"linear": CURVE_LINEAR, "basic": CURVE_BASIC, "deadzone": CURVE_DEADZONE, "table": CURVE_TABLE}
_CURVE_PRES = {"none": CURVE_PRE_NONE, "poly": CURVE_PRE_POLY, "table": CURVE_PRE_TABLE}
_CURVE_PARTS = {"command": CURVE_PART_COMMAND, "thrust": CURVE_PART_THRUST, "both": CURVE_PART_BOTH}
_CURVE_WHICH = {"curve": CURVE_WHICH_CURVE, "pre": CURVE_WHICH_PRE}


class _Opts(C.Structure):
    _fields_ = [("N", C.c_int32), ("qp_iter_max", C.c_int32), ("Ts", C.c_double), ("W", C.c_double * 16),
                ("We", C.c_double * 12), ("lbu", C.c_double * 4), ("ubu", C.c_double * 4), ("qp_tol_mu", C.c_double),
                ("qp_tol_stat", C.c_double), ("qp_early_exit", C.c_int32), ("kernel_path", C.c_int32),
                ("on_failure", C.c_int32), ("reserved_", C.c_int32)]


def library_path():
    return _LIB


def build_library(force=False):
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src = os.path.join(HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-s", "-C", src, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", src, "all"])
    return _LIB


_lib = None
_bound = set()


def _bind(L, table, restype=C.c_int):
    """prototypes of the entry points in `table` (name -> argtypes), all returning `restype`"""
    for name, args in table.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = restype


def _load(protos=None):
    """the library, loaded once; `protos(L)` -- a component's prototypes -- declared once"""
    global _lib
    if _lib is None:
        # PyTorch (device memory, streams, torch.distributed) ships its own HIP runtime; it has to be the first one mapped
        # into the process or hipGetDeviceCount() of a second runtime copy reports no device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(_LIB):
            raise FileNotFoundError(f"{_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "(the HIP extension is the only compute path; there is no fallback)")
        _lib = C.CDLL(_LIB)
    for f in (_protos, protos):
        if f is not None and f not in _bound:
            f(_lib)
            _bound.add(f)
    return _lib


def _protos(L):
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.brov_default_opts.argtypes = [C.POINTER(_Opts), C.c_int, C.c_double]
    L.brov_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(_Opts)]
    _bind(L, {"brov_last_error": []}, C.c_char_p)
    _bind(L, {"brov_destroy": [vp]}, None)
    _bind(L, {"brov_device_bytes": [vp]}, C.c_size_t)
    _bind(L, {"brov_plant_wrench_tick": [vp]}, C.c_int64)
    _bind(L, {name: [vp] for name in ("brov_results_device", "brov_x0_device", "brov_yref_device", "brov_params_device", "brov_x_device",
                                      "brov_u_device")}, vp)
    _bind(L, {
        "brov_set_x0_host": [vp, dp], "brov_set_x0_device": [vp, vp, vp],
        "brov_set_yref_host": [vp, dp, C.c_int], "brov_set_yref_device": [vp, vp, C.c_int, vp],
        "brov_set_params_host": [vp, dp, C.c_int], "brov_set_params_device": [vp, vp, C.c_int, vp],
        "brov_set_param_stage_host": [vp, C.c_int, C.c_int, dp],
        "brov_set_yref_stage_host": [vp, C.c_int, C.c_int, dp, C.c_int],
        "brov_set_iterate_host": [vp, dp, dp, dp, dp], "brov_get_iterate_host": [vp, dp, dp, dp, dp],
        "brov_set_opts": [vp, vp], "brov_get_opts": [vp, vp],
        "brov_reset": [vp], "brov_init_iterate_default": [vp], "brov_last_kernel_path": [vp], "brov_window_stages": [vp], "brov_lds_kernel_info": [vp, vp], "brov_solve": [vp, vp], "brov_synchronize": [vp, vp],
        "brov_get_results_host": [vp, vp], "brov_get_u0_host": [vp, dp],
        "brov_get_linearisation_host": [vp, dp, dp], "brov_select_best_host": [vp, ip, vp],
        "brov_get_thrusts_host": [vp, dp], "brov_last_solve_seconds": [vp, dp, dp], "brov_enable_timing": [vp, C.c_int],
        "brov_selftest_tile_tn": [dp, dp, dp, dp, C.c_int],
        "brov_selftest_sweep12": [dp, dp, C.POINTER(C.c_int)],
        "brov_selftest_model": [dp, dp, dp, dp, C.c_int],
        "brov_plant_set_params_host": [vp, dp], "brov_plant_step": [vp, C.c_double, C.c_int, vp], "brov_get_x0_host": [vp, dp],
        "brov_closed_loop": [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int32)],
        "brov_traj_set_host": [vp, dp, C.c_int], "brov_traj_rows": [vp], "brov_set_yref_from_traj": [vp, C.c_int, C.c_int, vp],
        "brov_set_yref_from_traj_lines_host": [vp, C.POINTER(C.c_int32), C.c_int],
        "brov_set_yref_candidates_host": [vp, C.c_int, dp, dp, dp, C.c_double, C.c_double],
        "brov_set_candidate_params_host": [vp, C.c_int, dp, dp, dp], "brov_set_yref_candidates": [vp, C.c_double, C.c_double, vp],
        "brov_debug_dump_linearisation": [vp, C.c_int], "brov_get_yref_host": [vp, dp], "brov_get_params_host": [vp, dp],
        "brov_tick_host": [vp, dp, dp, dp, C.c_int, vp],
        "brov_tick_buffers": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)],
        "brov_pit_last": [vp, C.POINTER(C.c_int32)], "brov_dev_reload_knobs": [vp], "brov_dev_tick_breakdown": [vp, dp], "brov_solve_ticks": [vp, vp, C.c_int, C.c_int, vp],
        "brov_set_time_steps": [vp, dp], "brov_set_stage0_weight": [vp, dp], "brov_general_grid": [vp],
        "brov_enable_dist6": [vp, C.c_int], "brov_dist6_enabled": [vp], "brov_set_rp_disturbance_host": [vp, dp, C.c_int],
        "brov_set_params18_host": [vp, dp, C.c_int], "brov_plant_set_rp_disturbance_host": [vp, dp], "brov_get_rp_disturbance_host": [vp, dp],
        "brov_plant_wrench_constant_host": [vp, dp], "brov_plant_wrench_periodic": [vp, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double],
        "brov_plant_wrench_table_host": [vp, dp, C.c_int, dp], "brov_plant_wrench_off": [vp], "brov_plant_wrench_mode": [vp],
        "brov_plant_wrench_seek": [vp, C.c_int64], "brov_plant_wrench_eval_host": [vp, C.c_int64, dp],
        "brov_closed_loop_ex": [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int32), dp],
        "brov_closed_loop_dob": [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int32), dp, dp],
        "brov_thruster_set_host": [vp, dp, dp, dp, dp, dp, C.POINTER(C.c_int64)], "brov_thruster_off": [vp], "brov_thruster_enabled": [vp],
        "brov_thruster_eval_host": [vp, C.c_int64, dp, dp, dp], "brov_thruster_last_host": [vp, dp],
        "brov_thruster_get_stats_host": [vp, C.POINTER(C.c_int32), dp, C.POINTER(C.c_int64)], "brov_thruster_reset_stats": [vp],
        "brov_thruster_last_seconds": [vp, dp],
        "brov_sensor_set_host": [vp, C.c_uint64, dp, dp, dp, C.POINTER(C.c_int32), dp], "brov_sensor_off": [vp], "brov_sensor_enabled": [vp],
        "brov_sensor_measure": [vp, vp], "brov_sensor_eval_host": [vp, C.c_int64, dp, dp, C.POINTER(C.c_int32)],
        "brov_sensor_get_measurement_host": [vp, dp], "brov_sensor_get_stats_host": [vp, C.POINTER(C.c_int32), dp, C.POINTER(C.c_int64)],
        "brov_sensor_reset_stats": [vp], "brov_sensor_last_seconds": [vp, dp],
        "brov_imu_set_host": [vp, C.POINTER(ImuParams), dp, dp, dp], "brov_imu_off": [vp], "brov_imu_enabled": [vp], "brov_imu_restart": [vp, vp],
        "brov_imu_eval_host": [vp, C.c_int64, dp, dp, dp, C.POINTER(C.c_int32), dp, dp, dp, dp, C.POINTER(C.c_int32)],
        "brov_imu_get_host": [vp, dp, dp, dp, dp, C.POINTER(C.c_int32)], "brov_imu_get_stats_host": [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64)],
        "brov_imu_reset_stats": [vp], "brov_imu_last_seconds": [vp, dp],
        "brov_current_constant_host": [vp, dp], "brov_current_table_host": [vp, dp, C.c_int, dp],
        "brov_current_gauss_markov_host": [vp, C.c_uint64, dp, dp, dp, dp, dp, C.c_double], "brov_current_off": [vp], "brov_current_mode": [vp],
        "brov_current_eval_host": [vp, C.c_int64, dp], "brov_current_get_state_host": [vp, dp], "brov_current_set_state_host": [vp, dp],
        "brov_current_last_host": [vp, dp], "brov_current_last_seconds": [vp, dp],
        "brov_coriolis_set": [vp, C.c_int, C.c_double, C.c_double], "brov_coriolis_off": [vp], "brov_coriolis_terms": [vp],
        "brov_coriolis_get": [vp, C.POINTER(C.c_int), dp, dp], "brov_coriolis_eval_host": [vp, dp, dp, dp], "brov_coriolis_last_host": [vp, dp],
        "brov_coriolis_last_seconds": [vp, dp],
        "brov_delay_set_host": [vp, C.POINTER(C.c_int32), C.c_int32, C.c_double, C.c_int32], "brov_delay_off": [vp], "brov_delay_enabled": [vp],
        "brov_delay_comp": [vp], "brov_delay_depth": [vp], "brov_delay_reset": [vp], "brov_delay_last_host": [vp, dp, dp],
        "brov_delay_queue_host": [vp, dp], "brov_delay_predict_host": [vp, dp, dp], "brov_delay_predicted_host": [vp, dp],
        "brov_delay_last_seconds": [vp, dp, dp],
        "brov_rotor_coeffs": [C.c_double, C.c_double, dp, dp], "brov_rotor_set_host": [vp, dp, C.c_double, dp, dp, C.c_int32],
        "brov_rotor_off": [vp], "brov_rotor_enabled": [vp], "brov_rotor_reset": [vp], "brov_rotor_set_state_host": [vp, dp],
        "brov_rotor_get_state_host": [vp, dp], "brov_rotor_last_host": [vp, dp, dp], "brov_rotor_get_stats_host": [vp, dp, C.POINTER(C.c_int64)],
        "brov_rotor_get_coeffs_host": [vp, dp, dp, dp], "brov_rotor_eval_host": [vp, dp, dp, dp, dp], "brov_rotor_last_seconds": [vp, dp],
        "brov_curve_set_table_host": [vp, C.c_int32, dp, dp, dp, C.c_int32],
        "brov_curve_get_table_host": [vp, C.c_int32, dp, dp, dp, dp, dp, C.POINTER(C.c_int32)],
        "brov_curve_set_host": [vp, C.POINTER(CurveParams), dp], "brov_curve_off": [vp], "brov_curve_enabled": [vp], "brov_curve_reset": [vp],
        "brov_curve_eval_host": [vp, C.c_int32, dp, dp, dp], "brov_curve_last_host": [vp, dp, dp, dp, dp],
        "brov_curve_get_stats_host": [vp, dp, C.POINTER(C.c_int32), dp, C.POINTER(C.c_int64)], "brov_curve_reset_stats": [vp],
        "brov_curve_last_seconds": [vp, dp, dp],
    })
    _bind(L, {"brov_thruster_default_matrix": [dp], "brov_imu_default_params": [C.POINTER(ImuParams)],
              "brov_curve_default_params": [C.POINTER(CurveParams)]}, None)
    _inspect.protos(_bind, L)
    _mesh.protos(_bind, L)


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _arr(a, shape, dtype=np.float64):
    """a mandatory array argument, contiguous, of exactly `shape`"""
    if a is None:
        raise ValueError(f"expected an array of shape {tuple(shape)}, got None")
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.shape != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
    return a


def _arr_opt(a, shape):
    """an optional array argument: None stays None (a null pointer in C)"""
    return None if a is None else _arr(a, shape)


class _Handle:
    """A device object of the C ABI (brov_solver, brov_ekf, brov_rls, brov_track, brov_group): its handle, the library, the name of the
    component's own *_last_error, and what every wrapper does with them."""
    _h = None
    _L = None
    _last_error = "brov_last_error"
    _destroy = "brov_destroy"

    def _error_text(self):
        return getattr(self._L, self._last_error)().decode()

    def _create(self, L, fn, *args, what=None):
        """self._h from the create call `fn(&handle, *args)`; without a usable device NoDeviceError"""
        self._L = L
        h = C.c_void_p()
        rc = getattr(L, fn)(C.byref(h), *args)
        if rc == -2:
            raise NoDeviceError(self._error_text() or "no HIP device")
        if rc != 0:
            raise RuntimeError(f"{what or fn} failed ({rc}): {self._error_text()}")
        self._h = h

    def close(self):
        if self._h:
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self._error_text()}")


class SolverOptions:
    """Defaults = the values baked into the reference's generated solver (acados_solver_bluerov2.c:389-669)."""

    def __init__(self, N=20, Ts=None, **kw):
        self._o = _Opts()
        _load().brov_default_opts(C.byref(self._o), int(N), float(1.0 / N if Ts is None else Ts))
        for k, v in kw.items():
            self.set(k, v)

    def set(self, k, v):
        if k in ("W", "We", "lbu", "ubu"):
            arr = getattr(self._o, k)
            if len(v) != len(arr):
                raise ValueError(f"{k} needs {len(arr)} values")
            for i, x in enumerate(v):
                arr[i] = float(x)
        elif hasattr(self._o, k):
            setattr(self._o, k, v)
        else:
            raise AttributeError(k)

    def __getattr__(self, k):
        o = object.__getattribute__(self, "_o")
        v = getattr(o, k)
        return np.array(v[:]) if k in ("W", "We", "lbu", "ubu") else v


def thrust_allocation(u0):
    """6 thruster commands from the 4 wrench commands (bluerov2_dob.cpp:390-395)."""
    u0 = np.asarray(u0, dtype=np.float64)
    c = ROTOR_CONSTANT
    return np.stack([(-u0[..., 0] + u0[..., 1] + u0[..., 3]) / c, (-u0[..., 0] - u0[..., 1] - u0[..., 3]) / c,
                     (u0[..., 0] + u0[..., 1] - u0[..., 3]) / c, (u0[..., 0] - u0[..., 1] + u0[..., 3]) / c,
                     -u0[..., 2] / c, -u0[..., 2] / c], axis=-1)


def rotor_coeffs(tau, h):
    """(alpha, beta) = (exp(-h / tau), (1 - alpha) / (h / tau)) of the rotor stage for the time constant tau and the step h, as the library's
    host code computes and uploads them (brov_rotor_coeffs; tau == 0: (0, 0)); needs no GPU"""
    al, be = C.c_double(0.0), C.c_double(0.0)
    rc = _load().brov_rotor_coeffs(float(tau), float(h), C.byref(al), C.byref(be))
    if rc != 0:
        raise ValueError(f"rotor_coeffs({tau}, {h}): tau must be finite and >= 0, h finite and > 0")
    return al.value, be.value


def curve_from_pwm_table(pwm, kgf, amps=None, neutral=1500.0):
    """(x, y, amps): a thruster's measured table (PWM in microseconds, force, current; the columns of tests/golden/t200_16v.json) as a curve table
    of the thrust-curve stage.  The abscissa is pwm - neutral, so that a command of 0 -- the rotor stage's zero state -- is a stopped
    thruster; the ordinates stay in the table's units (eff carries the change to what K multiplies).  Needs no device."""
    x = np.asarray(pwm, dtype=np.float64) - float(neutral)
    y = np.array(kgf, dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape or len(x) < 2 or not np.all(np.diff(x) > 0):
        raise ValueError("pwm must be one strictly increasing column of at least two rows, kgf one of the same length")
    a = None if amps is None else np.array(amps, dtype=np.float64)
    if a is not None and a.shape != x.shape:
        raise ValueError("amps must have the length of pwm")
    return x, y, a


def inverse_table(x, y):
    """(y', x'): the table (x, y) with its columns swapped, as a pre-map that undoes the curve, after dropping every knot whose ordinate
    does not exceed the last kept one, so that the new abscissae increase strictly.  Of a dead band -- a run of equal ordinates -- only
    its FIRST knot survives: the inverse answers a wanted thrust of exactly 0 with the command at the band's lower edge, jumps across the
    whole band to the first knot beyond it for the smallest positive thrust, and so never asks for a command inside the band; the curve
    applied to it is the identity on the table's range up to the interpolation error of one table step, but a command that a quantisation
    rounds back into the band is lost.  A non-monotone stretch of the curve is dropped likewise.  Needs no device."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape or len(x) < 2:
        raise ValueError("x and y must be two columns of one length >= 2")
    keep = [0]
    for j in range(1, len(y)):
        if y[j] > y[keep[-1]]:
            keep.append(j)
    if len(keep) < 2:
        raise ValueError("the table has no two increasing ordinates")
    return y[keep].copy(), x[keep].copy()


def current_from_angles(speed, horizontal, vertical):
    """world-frame current (vx, vy, vz) from speed V and the horizontal and vertical angles h, v in radians, the convention of the
    reference's underwater_current_plugin: (V cos h cos v, V sin h cos v, V sin v); broadcasts, the components on the last axis"""
    V, h, v = np.broadcast_arrays(np.asarray(speed, dtype=np.float64), np.asarray(horizontal, dtype=np.float64),
                                  np.asarray(vertical, dtype=np.float64))
    return np.stack([V * np.cos(h) * np.cos(v), V * np.sin(h) * np.cos(v), V * np.sin(v)], axis=-1)


class _Wrench:
    """The world-frame wrench generator of `owner` through the entry points `prefix`* of the C ABI, written once for BatchSolver
    (brov_plant_wrench_, one wrench per instance) and Fleet (brov_vehicle_wrench_, one per vehicle): `batch` wrenches, `name` the owner's
    public setter, which the texts of the exceptions cite.  Made per call: it keeps the owner alive no longer than that."""

    def __init__(self, owner, prefix, batch, name):
        self.o, self.prefix, self.batch, self.name = owner, prefix, batch, name

    def call(self, op, *args):   # a failure is reported as e.g. "plant_wrench_constant failed (-1): ..."
        self.o._chk(getattr(self.o._L, self.prefix + op)(self.o._h, *args), self.name[4:] + "_" + op.replace("_host", ""))

    def set(self, constant, periodic, table, gain):
        if (constant is not None) + (periodic is not None) + (table is not None) != 1:
            raise ValueError(f"{self.name} takes exactly one of constant=, periodic=, table=")
        if gain is not None and table is None:
            raise ValueError("gain= goes with table=")
        if constant is not None:
            w = np.asarray(constant, dtype=np.float64)   # one wrench [6] for all, or [batch, 6]
            self.call("constant_host", _dp(_arr(np.broadcast_to(w, (self.batch, 6)) if w.shape == (6,) else w, (self.batch, 6))))
        elif periodic is not None:
            kw = dict(seed=0, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)
            unknown = set(periodic) - set(kw)
            if unknown:
                raise ValueError(f"unknown periodic wrench parameters {sorted(unknown)}")
            kw.update(periodic)
            self.call("periodic", int(kw["seed"]) & 0xFFFFFFFFFFFFFFFF, float(kw["scale"]), float(kw["phase0"]), float(kw["dphi"]), float(kw["tz_div"]))
        else:
            tab = np.ascontiguousarray(table, dtype=np.float64)
            if tab.ndim != 2 or tab.shape[1] != 6 or tab.shape[0] < 1:
                raise ValueError("wrench table must be [rows][6]")
            self.call("table_host", _dp(tab), tab.shape[0], _dp(_arr_opt(gain, (self.batch,))))

    def get(self, what):   # "mode" or "tick"
        return int(getattr(self.o._L, self.prefix + what)(self.o._h))

    def eval(self, tick):
        w = np.empty((self.batch, 6))
        self.call("eval_host", int(tick), _dp(w))
        return w


class BatchSolver(_Handle):
    """B independent BlueROV2 OCP instances resident on one GPU; one solve() = one RTI step of each."""

    def __init__(self, batch, opts=None, device=0):
        L = _load()
        self.opts = opts if opts is not None else SolverOptions()
        self.B, self.N = int(batch), int(self.opts.N)
        self._create(L, "brov_create", int(device), self.B, C.byref(self.opts._o))
        self.device = int(device)

    def set_options(self, opts):
        """change weights / bounds / limits / policies at run time (brov_set_opts; the horizon is fixed at create)"""
        self._chk(self._L.brov_set_opts(self._h, C.byref(opts._o)), "set_opts")
        self.opts = opts

    @property
    def device_bytes(self):
        return int(self._L.brov_device_bytes(self._h))

    # ---- inputs (host numpy) --------------------------------------------------------------------------------
    def set_x0(self, x0):
        self._chk(self._L.brov_set_x0_host(self._h, _dp(_arr(x0, (self.B, NX)))), "set_x0")

    def set_yref(self, yref):
        yref = np.ascontiguousarray(yref, dtype=np.float64)
        if yref.shape == (self.N + 1, NY):
            self._chk(self._L.brov_set_yref_host(self._h, _dp(yref), 1), "set_yref")
        else:
            self._chk(self._L.brov_set_yref_host(self._h, _dp(_arr(yref, (self.B, self.N + 1, NY))), 0), "set_yref")

    def set_params(self, p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        if p.shape == (NP,):
            p = np.ascontiguousarray(np.broadcast_to(p, (self.B, NP)))
        if p.shape == (self.B, NP):
            self._chk(self._L.brov_set_params_host(self._h, _dp(p), 0), "set_params")
        else:
            self._chk(self._L.brov_set_params_host(self._h, _dp(_arr(p, (self.B, self.N + 1, NP))), 1), "set_params")

    # ---- inputs (device pointers, e.g. torch tensors' data_ptr()) ---------------------------------------------
    def set_x0_device(self, ptr, stream=0):
        self._chk(self._L.brov_set_x0_device(self._h, C.c_void_p(ptr), C.c_void_p(stream)), "set_x0_device")

    def set_yref_device(self, ptr, shared, stream=0):
        self._chk(self._L.brov_set_yref_device(self._h, C.c_void_p(ptr), int(bool(shared)), C.c_void_p(stream)), "set_yref_device")

    def set_params_device(self, ptr, per_stage, stream=0):
        self._chk(self._L.brov_set_params_device(self._h, C.c_void_p(ptr), int(bool(per_stage)), C.c_void_p(stream)), "set_params_device")

    # ---- reference windows built on the device (bluerov2_path.cpp:79-118 semantics) ---------------------------
    def set_trajectory(self, traj):
        traj = np.ascontiguousarray(traj, dtype=np.float64)
        if traj.ndim != 2 or traj.shape[1] != NY:
            raise ValueError("trajectory must be [rows][16]")
        self._chk(self._L.brov_traj_set_host(self._h, _dp(traj), traj.shape[0]), "set_trajectory")

    def set_yref_from_trajectory(self, line, ncols=16, stream=0):
        """line: int -> one shared window; array[B] -> per-instance windows"""
        if np.ndim(line) == 0:
            self._chk(self._L.brov_set_yref_from_traj(self._h, int(line), int(ncols), C.c_void_p(stream)), "set_yref_from_traj")
        else:
            lines = np.ascontiguousarray(line, dtype=np.int32)
            if lines.shape != (self.B,):
                raise ValueError("lines must be [B]")
            self._chk(self._L.brov_set_yref_from_traj_lines_host(self._h, lines.ctypes.data_as(C.POINTER(C.c_int32)), int(ncols)),
                      "set_yref_from_traj_lines")

    def set_yref_candidates(self, kind, p0, p1, phase, t0=0.0, dt=0.05):
        k = {"lemniscate": 0, "circle": 1}[kind]
        a, b, c = (_arr(v, (self.B,)) for v in (p0, p1, phase))
        self._chk(self._L.brov_set_yref_candidates_host(self._h, k, _dp(a), _dp(b), _dp(c), float(t0), float(dt)), "set_yref_candidates")

    def set_candidate_params(self, kind, p0, p1, phase):
        """shape parameters stay on the device; set_yref_candidates_tick() then rebuilds the windows without host traffic"""
        k = {"lemniscate": 0, "circle": 1}[kind]
        a, b, c = (_arr(v, (self.B,)) for v in (p0, p1, phase))
        self._chk(self._L.brov_set_candidate_params_host(self._h, k, _dp(a), _dp(b), _dp(c)), "set_candidate_params")

    def set_yref_candidates_tick(self, t0, dt=0.05, stream=0):
        self._chk(self._L.brov_set_yref_candidates(self._h, float(t0), float(dt), C.c_void_p(stream)), "set_yref_candidates_tick")

    def get_yref(self):
        y = np.empty((self.B, self.N + 1, NY))
        self._chk(self._L.brov_get_yref_host(self._h, _dp(y)), "get_yref")
        return y

    # ---- closed loop on the device ---------------------------------------------------------------
    def tick(self, x0=None, yref=None, params=None, rti_phase=0):
        """one control tick with ONE host wait (brov_tick_host): the inputs that changed (None = unchanged; x0 [B,12], ONE reference
        window shared by the batch [N+1,16], per-stage parameters [B,N+1,16]) + the step + the result records"""
        res = np.zeros(self.B, dtype=RESULT_DTYPE)
        a, b, c = _arr_opt(x0, (self.B, NX)), _arr_opt(yref, (self.N + 1, NY)), _arr_opt(params, (self.B, self.N + 1, NP))
        self._chk(self._L.brov_tick_host(self._h, _dp(a), _dp(b), _dp(c), int(rti_phase), C.c_void_p(res.ctypes.data)), "tick")
        return res

    def solve_ticks(self, ticks, row_stride=0, stream=None, status_log_ptr=None, sync=False):
        """`ticks` RTI steps in one call (brov_solve_ticks): one launch on the fused kernels, every instance on to its next step when its own is
        done; the shared window moves on row_stride rows of the resident trajectory per step"""
        self._chk(self._L.brov_solve_ticks(self._h, C.c_void_p(stream or 0), int(ticks), int(row_stride), C.c_void_p(status_log_ptr or 0)), "solve_ticks")
        if sync:
            self._chk(self._L.brov_synchronize(self._h, C.c_void_p(stream or 0)), "synchronize")

    def tick_breakdown(self):
        """development (BROV_TICK_BREAKDOWN=1 at create): host microseconds of the last tick -- staging, launch, post-launch, wait, total"""
        us = np.zeros(5)
        self._chk(self._L.brov_dev_tick_breakdown(self._h, _dp(us)), "tick_breakdown")
        return us

    def reload_knobs(self):
        """development: the solver reads its BROV_* environment knobs once, at create; a test that flips one between two solves of the
        same solver calls this (brov_dev_reload_knobs)"""
        self._chk(self._L.brov_dev_reload_knobs(self._h), "reload_knobs")

    def pit_last(self):
        """[B] int32: 1 where the parallel-in-time kernel completed the instance's last step (resident windowed mode only)"""
        d = np.zeros(self.B, dtype=np.int32)
        self._chk(self._L.brov_pit_last(self._h, d.ctypes.data_as(C.POINTER(C.c_int32))), "pit_last")
        return d

    def tick_buffers(self):
        """numpy views of brov_tick_host's pinned staging buffers (brov_tick_buffers): dict(x0 [B,12], yref [N+1,16], params [B,N+1,16],
        results [B] records).  Fill the inputs in place, call tick_inplace(), read `results` in place: no host-side copies."""
        if getattr(self, "_tick_views", None) is None:
            p = [C.c_void_p() for _ in range(4)]
            self._chk(self._L.brov_tick_buffers(self._h, *[C.byref(q) for q in p]), "tick_buffers")

            def view(ptr, shape, dtype=np.float64):
                n = int(np.prod(shape)) * np.dtype(dtype).itemsize
                return np.frombuffer((C.c_char * n).from_address(ptr.value), dtype=dtype).reshape(shape)
            self._tick_ptrs = [C.cast(q, C.POINTER(C.c_double)) for q in p[:3]]
            self._tick_views = dict(x0=view(p[0], (self.B, NX)), yref=view(p[1], (self.N + 1, NY)), params=view(p[2], (self.B, self.N + 1, NP)),
                                    results=view(p[3], (self.B,), RESULT_DTYPE))
        return self._tick_views

    def tick_inplace(self, x0=True, yref=True, params=False, rti_phase=0):
        """brov_tick_host on the staging buffers themselves: which of the inputs the caller has rewritten there; returns the results view"""
        v = self.tick_buffers()
        p = self._tick_ptrs
        self._chk(self._L.brov_tick_host(self._h, p[0] if x0 else None, p[1] if yref else None, p[2] if params else None, int(rti_phase), None), "tick")
        return v["results"]

    # ---- non-uniform grid / separate stage-0 weight (acados_solver_bluerov2.h:141,146; .c:422-441): streaming kernels ------------
    def set_time_steps(self, ts):
        self._chk(self._L.brov_set_time_steps(self._h, _dp(_arr_opt(ts, (self.N,)))), "set_time_steps")

    def set_stage0_weight(self, W0):
        self._chk(self._L.brov_set_stage0_weight(self._h, _dp(_arr_opt(W0, (NY,)))), "set_stage0_weight")

    # ---- 6-disturbance model variant: roll / pitch disturbance moments next to p[16] ---------------------
    def enable_dist6(self, on=True):
        self._chk(self._L.brov_enable_dist6(self._h, int(bool(on))), "enable_dist6")

    def set_rp_disturbance(self, d):
        """d: [2] / [B, 2] (constant over the horizon) or [B, N+1, 2] (per stage): d_phi, d_theta"""
        d = np.ascontiguousarray(d, dtype=np.float64)
        if d.shape == (2,):
            d = np.ascontiguousarray(np.broadcast_to(d, (self.B, 2)))
        if d.shape == (self.B, 2):
            self._chk(self._L.brov_set_rp_disturbance_host(self._h, _dp(d), 0), "set_rp_disturbance")
        else:
            self._chk(self._L.brov_set_rp_disturbance_host(self._h, _dp(_arr(d, (self.B, self.N + 1, 2))), 1), "set_rp_disturbance")

    def get_rp_disturbance(self):
        d = np.empty((self.B, self.N + 1, 2))
        self._chk(self._L.brov_get_rp_disturbance_host(self._h, _dp(d)), "get_rp_disturbance")
        return d

    def set_params18(self, p18):
        """the parameter vector of the uncommented 6-disturbance model: [dx dy dz d_phi d_theta d_psi | 12 hydrodynamic], [B, 18] or
        [B, N+1, 18]"""
        p18 = np.ascontiguousarray(p18, dtype=np.float64)
        if p18.shape == (self.B, 18):
            self._chk(self._L.brov_set_params18_host(self._h, _dp(p18), 0), "set_params18")
        else:
            self._chk(self._L.brov_set_params18_host(self._h, _dp(_arr(p18, (self.B, self.N + 1, 18))), 1), "set_params18")

    def set_plant_rp_disturbance(self, d):
        self._chk(self._L.brov_plant_set_rp_disturbance_host(self._h, _dp(_arr_opt(d, (self.B, 2)))), "set_plant_rp_disturbance")

    def set_plant_params(self, p):
        self._chk(self._L.brov_plant_set_params_host(self._h, _dp(_arr(p, (self.B, NP)))), "set_plant_params")

    def get_params(self):
        """model parameters currently in force, [B, N+1, 16]"""
        p = np.empty((self.B, self.N + 1, NP))
        self._chk(self._L.brov_get_params_host(self._h, _dp(p)), "get_params")
        return p

    def plant_step(self, dt=0.05, substeps=1, stream=0):
        self._chk(self._L.brov_plant_step(self._h, float(dt), int(substeps), C.c_void_p(stream)), "plant_step")

    def get_x0(self):
        x0 = np.empty((self.B, NX))
        self._chk(self._L.brov_get_x0_host(self._h, _dp(x0)), "get_x0")
        return x0

    def closed_loop(self, ticks, line0=0, ncols=16, dt=0.05, substeps=1, log=True, log_wrench=False):
        """ticks x (window -> RTI step -> plant step) on the device; returns (u_log, x_log, status_log) or None; with log_wrench also the
        applied world-frame wrench of every tick, (u_log, x_log, status_log, w_log [ticks, B, 6])"""
        if not log and not log_wrench:
            self._chk(self._L.brov_closed_loop(self._h, int(ticks), int(line0), int(ncols), float(dt), int(substeps), None, None, None),
                      "closed_loop")
            return None
        ul, xl = np.empty((ticks, self.B, NU)), np.empty((ticks + 1, self.B, NX))
        sl = np.empty((ticks, self.B), dtype=np.int32)
        if not log_wrench:
            self._chk(self._L.brov_closed_loop(self._h, int(ticks), int(line0), int(ncols), float(dt), int(substeps), _dp(ul), _dp(xl),
                                               sl.ctypes.data_as(C.POINTER(C.c_int32))), "closed_loop")
            return ul, xl, sl
        wl = np.empty((ticks, self.B, 6))
        self._chk(self._L.brov_closed_loop_ex(self._h, int(ticks), int(line0), int(ncols), float(dt), int(substeps), _dp(ul), _dp(xl),
                                              sl.ctypes.data_as(C.POINTER(C.c_int32)), _dp(wl)), "closed_loop_ex")
        return ul, xl, sl, wl

    def closed_loop_dob(self, ekf, rls=None, rls_mode=0, ticks=1, line0=0, ncols=16, dt=0.05, substeps=1, log=True):
        """the DOB (rls None) / AMPC control loop on the device (brov_closed_loop_dob): ticks x (window -> RTI step -> plant step under
        the wrench in force -> EKF from the solver -> parameter hand-off), one host wait.  Returns dict(u, x, status, wrench, est) --
        est [ticks, B, 6]: the observer's disturbance estimate after each tick -- or None"""
        hr = rls._h if rls is not None else None
        args = (self._h, ekf._h, hr, int(rls_mode), int(ticks), int(line0), int(ncols), float(dt), int(substeps))
        if not log:
            self._chk(self._L.brov_closed_loop_dob(*args, None, None, None, None, None), "closed_loop_dob")
            return None
        ul, xl = np.empty((ticks, self.B, NU)), np.empty((ticks + 1, self.B, NX))
        sl = np.empty((ticks, self.B), dtype=np.int32)
        wl, el = np.empty((ticks, self.B, 6)), np.empty((ticks, self.B, 6))
        self._chk(self._L.brov_closed_loop_dob(*args, _dp(ul), _dp(xl), sl.ctypes.data_as(C.POINTER(C.c_int32)), _dp(wl), _dp(el)),
                  "closed_loop_dob")
        return dict(u=ul, x=xl, status=sl, wrench=wl, est=el)

    def closed_loop_track(self, track, ticks, line0=0, ncols=16, dt=0.05, substeps=1, ekf=None, rls=None, rls_mode=0, chunk=0):
        """the closed loop scored instead of logged (brov_closed_loop_track): the ticks of closed_loop() -- with ekf= those of closed_loop_dob(),
        rls= making it the AMPC loop -- in chunks of `chunk` ticks (0: 64), each chunk's device logs folded into `track` (a BatchTrack) against
        the trajectory table; one host wait, no host log.  The statistics continue those of earlier calls (track.reset() starts afresh)."""
        he = ekf._h if ekf is not None else None
        hr = rls._h if rls is not None else None
        self._chk(track._L.brov_closed_loop_track(self._h, he, hr, int(rls_mode), track._h, int(ticks), int(line0), int(ncols), float(dt),
                                                  int(substeps), int(chunk)), "closed_loop_track")

    # ---- time-varying world-frame wrench on the plant (bluerov2_dob.cpp:754-892, applyBodyWrench) ------------------------------
    _wrench = property(lambda self: _Wrench(self, "brov_plant_wrench_", self.B, "set_plant_wrench"))

    def set_plant_wrench(self, constant=None, periodic=None, table=None, gain=None):
        """exactly one of
            constant=w         [6] or [B, 6], world frame [fx fy fz tx ty tz]; the reference's mode 1 is (10, 10, 10, 0, 0, 0)
            periodic=dict(seed=0, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)   (any subset; dphi = 0.025 is the AMPC node's)
            table=tab          [rows, 6], row min(tick, rows - 1); gain=[B] scales it per instance"""
        self._wrench.set(constant, periodic, table, gain)

    def plant_wrench_off(self):
        self._wrench.call("off")

    def plant_wrench_mode(self):
        return self._wrench.get("mode")

    def plant_wrench(self, tick):
        """[B, 6]: the wrench of every instance at `tick`, evaluated by the device generator (moves nothing)"""
        return self._wrench.eval(tick)

    def plant_wrench_seek(self, tick):
        self._wrench.call("seek", int(tick))

    def plant_wrench_tick(self):
        """the tick counter: plant steps so far (plant_step and every closed-loop tick add one)"""
        return self._wrench.get("tick")

    # ---- thruster stage of the plant: limits, per-instance faults, propulsion matrix (brov_thruster_*) ---------------------------
    def set_thrusters(self, K=None, lo=None, hi=None, gain=None, bias=None, onset=None):
        """the plant steps from now on run behind the thruster stage, and its statistics start afresh.  With t the six commands of the result
        record (thrusts()): c = clamp(t, lo, hi);  a = gain * c + bias from tick onset[b] on, else c;  wrench [X Y Z K M N] = K a.
            K            [6, 6] rows = force axes, columns = thrusters (None: the model's own, thruster_matrix())
            lo, hi       scalar or [6], shared by the batch (None: no limit); the reference's thruster manager has -1540, 1540
            gain, bias   scalar, [6] or [B, 6] (None: 1, 0); a weak thruster is gain 0.5, a dead one 0, a stuck one gain 0 and bias c
            onset        scalar or [B], plant ticks (plant_wrench_tick()) from which gain and bias apply (None: 0)"""
        def rows(v, shape):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), shape))
        Ka = None if K is None else _arr(K, (6, 6))
        on = None if onset is None else np.ascontiguousarray(np.broadcast_to(np.asarray(onset, dtype=np.int64), (self.B,)))
        lo_, hi_, g_, b_ = rows(lo, (6,)), rows(hi, (6,)), rows(gain, (self.B, 6)), rows(bias, (self.B, 6))
        self._chk(self._L.brov_thruster_set_host(self._h, _dp(Ka), _dp(lo_), _dp(hi_), _dp(g_), _dp(b_),
                                                 None if on is None else on.ctypes.data_as(C.POINTER(C.c_int64))), "set_thrusters")

    def thrusters_off(self):
        """the plant kernels as they always were; the statistics stay readable"""
        self._chk(self._L.brov_thruster_off(self._h), "thrusters_off")

    def thrusters_enabled(self):
        return bool(self._L.brov_thruster_enabled(self._h))

    def thruster_eval(self, tick, commanded):
        """(applied [B, 6], wrench [B, 6]) of the stage alone for `commanded` [B, 6] at `tick`; moves no counter, touches no statistic"""
        c = _arr(commanded, (self.B, 6))
        a, g = np.empty((self.B, 6)), np.empty((self.B, 6))
        self._chk(self._L.brov_thruster_eval_host(self._h, int(tick), _dp(c), _dp(a), _dp(g)), "thruster_eval")
        return a, g

    def thruster_last(self):
        """[B, 6]: the thrusts the last plant step behind the stage applied"""
        a = np.empty((self.B, 6))
        self._chk(self._L.brov_thruster_last_host(self._h, _dp(a)), "thruster_last")
        return a

    def thruster_stats(self):
        """dict(clip_ticks [B, 6] int32: plant steps on which the command lay outside its limits; lost_sq [B]: running sum of
        |commanded - applied|^2; steps: plant steps behind the stage since the statistics were reset)"""
        clip, lost, steps = np.zeros((self.B, 6), dtype=np.int32), np.empty(self.B), C.c_int64(0)
        self._chk(self._L.brov_thruster_get_stats_host(self._h, clip.ctypes.data_as(C.POINTER(C.c_int32)), _dp(lost), C.byref(steps)),
                  "thruster_stats")
        return dict(clip_ticks=clip, lost_sq=lost, steps=int(steps.value))

    def thruster_reset_stats(self):
        self._chk(self._L.brov_thruster_reset_stats(self._h), "thruster_reset_stats")

    def thruster_last_seconds(self):
        """duration of the last plant kernel launched behind the stage (HIP events)"""
        sec = C.c_double(0.0)
        self._chk(self._L.brov_thruster_last_seconds(self._h, C.byref(sec)), "thruster_last_seconds")
        return sec.value

    @staticmethod
    def thruster_matrix():
        """[6, 6]: the model's own propulsion matrix, the default K"""
        K = np.empty((6, 6))
        _load().brov_thruster_default_matrix(_dp(K))
        return K

    # ---- delay stage between the commands and the plant, and the predictor ahead of the solve (brov_delay_*) ---------------------------------
    def set_delay(self, delay=None, comp=0, dt_pred=None, observer_applied=False):
        """the plant steps from now on are given the record commanded delay[b] steps earlier (zeros before the first); the queue and the stage's
        step count start afresh.
            delay             scalar or [B] in 0 ... 8 (None: 0), plant steps between a command and its arrival
            comp              0 ... 8, one number for the batch: every solve starts from the controller's state carried through the last `comp`
                              commanded inputs by its own model, and the closed loops start their windows comp rows ahead
            dt_pred           the predictor's step (None: the options' Ts)
            observer_applied  BatchEkf.update_from_solver reads the applied thrusts in place of the commanded ones"""
        d = None if delay is None else np.ascontiguousarray(np.broadcast_to(np.asarray(delay, dtype=np.int32), (self.B,)))
        self._chk(self._L.brov_delay_set_host(self._h, None if d is None else d.ctypes.data_as(C.POINTER(C.c_int32)), int(comp),
                                              0.0 if dt_pred is None else float(dt_pred), int(bool(observer_applied))), "set_delay")

    def delay_off(self):
        """every launch as it was without the stage; the queue stays readable"""
        self._chk(self._L.brov_delay_off(self._h), "delay_off")

    def delay_enabled(self):
        return bool(self._L.brov_delay_enabled(self._h))

    def delay_comp(self):
        return int(self._L.brov_delay_comp(self._h))

    def delay_depth(self):
        """D: slots of the queue, max(max delay, comp) + 1"""
        return int(self._L.brov_delay_depth(self._h))

    def delay_reset(self):
        """zeroes the queue and the stage's step count"""
        self._chk(self._L.brov_delay_reset(self._h), "delay_reset")

    def delay_last(self):
        """(u0 [B, 4], thrust [B, 6]): what the last plant step behind the stage was given"""
        u, t = np.empty((self.B, NU)), np.empty((self.B, 6))
        self._chk(self._L.brov_delay_last_host(self._h, _dp(u), _dp(t)), "delay_last")
        return u, t

    def delay_queue(self):
        """[B, D, 4]: the u0 of the last D commanded records, oldest first (zeros for steps before the first)"""
        q = np.empty((self.B, self.delay_depth(), NU))
        self._chk(self._L.brov_delay_queue_host(self._h, _dp(q)), "delay_queue")
        return q

    def delay_predict(self, y=None):
        """[B, 12]: the predictor alone from y [B, 12] (None: what the controller knows of the state); moves nothing"""
        out = np.empty((self.B, NX))
        self._chk(self._L.brov_delay_predict_host(self._h, _dp(_arr_opt(y, (self.B, NX))), _dp(out)), "delay_predict")
        return out

    def delay_predicted(self):
        """[B, 12]: the state the last solve started from (comp > 0)"""
        out = np.empty((self.B, NX))
        self._chk(self._L.brov_delay_predicted_host(self._h, _dp(out)), "delay_predicted")
        return out

    def delay_last_seconds(self):
        """(shift, predict): durations of the last launch of the stage's two kernels (HIP events); None where none was launched yet"""
        out = []
        for k in range(2):
            sec = C.c_double(0.0)
            args = (C.byref(sec), None) if k == 0 else (None, C.byref(sec))
            rc = self._L.brov_delay_last_seconds(self._h, *args)
            if rc != -1:                       # (BROV_ERR_ARG: that kernel has not been launched yet)
                self._chk(rc, "delay_last_seconds")
            out.append(sec.value if rc == 0 else None)
        return tuple(out)

    # ---- rotor stage between the commands and the plant: first-order dynamics of the thrusters (brov_rotor_*) ---------------------------------
    def set_rotors(self, tau=None, h=None, cmd_lo=None, cmd_hi=None, observer_applied=False):
        """the plant steps from now on are given the mean thrust of rotors that follow their commands with r' = (c - r) / tau; the rotor state,
        the statistics and the stage's step count start afresh.  The chain is delay -> rotors -> thruster stage -> model.
            tau               scalar, [6] or [B, 6] seconds, >= 0 (None: 0.2, the reference's; 0: that rotor follows at once)
            h                 the plant step the coefficients are computed for (None: the options' Ts); plant steps of another dt are refused
            cmd_lo, cmd_hi    scalar or [6], limits of the commands ahead of the dynamics (None: none)
            observer_applied  BatchEkf.update_from_solver reads the applied (lagged) thrusts in place of the commanded ones"""
        t = None if tau is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tau, dtype=np.float64), (self.B, 6)))
        lo = None if cmd_lo is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cmd_lo, dtype=np.float64), (6,)))
        hi = None if cmd_hi is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cmd_hi, dtype=np.float64), (6,)))
        self._chk(self._L.brov_rotor_set_host(self._h, _dp(t), 0.0 if h is None else float(h), _dp(lo), _dp(hi), int(bool(observer_applied))),
                  "set_rotors")

    def rotor_off(self):
        """every launch as it was without the stage; state and statistics stay readable"""
        self._chk(self._L.brov_rotor_off(self._h), "rotor_off")

    def rotor_enabled(self):
        return bool(self._L.brov_rotor_enabled(self._h))

    def rotor_reset(self):
        """zeroes the rotor state, the statistics and the stage's step count"""
        self._chk(self._L.brov_rotor_reset(self._h), "rotor_reset")

    def rotor_state(self):
        """[B, 6]: the thrust every rotor gives at the end of the last step"""
        r = np.empty((self.B, 6))
        self._chk(self._L.brov_rotor_get_state_host(self._h, _dp(r)), "rotor_state")
        return r

    def set_rotor_state(self, r):
        self._chk(self._L.brov_rotor_set_state_host(self._h, _dp(_arr(r, (self.B, 6)))), "set_rotor_state")

    def rotor_last(self):
        """(u0 [B, 4], thrust [B, 6]): what the last plant step behind the stage was given"""
        u, t = np.empty((self.B, NU)), np.empty((self.B, 6))
        self._chk(self._L.brov_rotor_last_host(self._h, _dp(u), _dp(t)), "rotor_last")
        return u, t

    def rotor_stats(self):
        """dict(lag_sq [B]: running sum of |command - applied|^2; steps: steps of the stage since it was set or reset)"""
        lag, steps = np.empty(self.B), C.c_int64(0)
        self._chk(self._L.brov_rotor_get_stats_host(self._h, _dp(lag), C.byref(steps)), "rotor_stats")
        return dict(lag_sq=lag, steps=int(steps.value))

    def rotor_coeffs(self):
        """dict(alpha [B, 6], beta [B, 6], h): the coefficients the stage uploaded and the step they hold for"""
        al, be, h = np.empty((self.B, 6)), np.empty((self.B, 6)), C.c_double(0.0)
        self._chk(self._L.brov_rotor_get_coeffs_host(self._h, _dp(al), _dp(be), C.byref(h)), "rotor_coeffs")
        return dict(alpha=al, beta=be, h=h.value)

    def rotor_eval(self, commanded, state=None):
        """(applied [B, 6], new state [B, 6]) of the stage alone for `commanded` [B, 6] from `state` [B, 6] (None: the stage's own); moves nothing"""
        c = _arr(commanded, (self.B, 6))
        a, r = np.empty((self.B, 6)), np.empty((self.B, 6))
        self._chk(self._L.brov_rotor_eval_host(self._h, _dp(c), _dp(_arr_opt(state, (self.B, 6))), _dp(a), _dp(r)), "rotor_eval")
        return a, r

    def rotor_last_seconds(self):
        """duration of the last shift launch (HIP events); None where none was launched yet"""
        sec = C.c_double(0.0)
        rc = self._L.brov_rotor_last_seconds(self._h, C.byref(sec))
        if rc != -1:                           # (BROV_ERR_ARG: no plant step behind the stage yet)
            self._chk(rc, "rotor_last_seconds")
        return sec.value if rc == 0 else None

    # ---- thrust-curve stage around the rotors: command map and ESC steps ahead, conversion curve and efficiency behind (brov_curve_*) ----------
    def thrust_curve_table(self, which="curve", x=None, y=None, amps=None):
        """with x and y: sets the table `which` ("curve" or "pre"; amps: the curve table's third column), which holds from the next plant
        step on.  Returns dict(x, y, slope, amps, amps_slope) of [K] each: the values the stage uploaded (K = 0: no table set)"""
        w = _CURVE_WHICH[which] if isinstance(which, str) else int(which)
        if x is not None:
            xa = np.ascontiguousarray(x, dtype=np.float64).ravel()
            ya = _arr(y, xa.shape)
            self._chk(self._L.brov_curve_set_table_host(self._h, w, _dp(xa), _dp(ya), _dp(_arr_opt(amps, xa.shape)), len(xa)), "thrust_curve_table")
        cols = [np.zeros(CURVE_MAX_KNOTS) for _ in range(5)]
        K = C.c_int32(0)
        self._chk(self._L.brov_curve_get_table_host(self._h, w, *[_dp(c) for c in cols], C.byref(K)), "thrust_curve_table")
        return dict(zip(("x", "y", "slope", "amps", "amps_slope"), (c[:K.value].copy() for c in cols)))

    def set_thrust_curve(self, kind="linear", pre="none", quantum=0.0, k=1.0, kl=1.0, kr=1.0, dl=0.0, dr=0.0, pre_poly=None, eff=None,
                         observer_applied=False):
        """the plant steps from now on turn the commanded thrusts into force through the thrust-curve stage; its books start afresh.  The chain
        is delay -> [pre-map, quantisation] -> rotors -> [conversion, efficiency] -> thruster stage -> model.
            kind      "linear" (a copy), "basic" (k w |w|), "deadzone" (kl (v - dl) / 0 / kr (v - dr) of v = w |w|) or "table" (thrust_curve_table)
            pre       "none", "poly" (pre_poly [5], highest degree first) or "table" (thrust_curve_table("pre", ...))
            quantum   step of the command behind the pre-map (0: none)
            eff       scalar, [6] or [B, 6] (None: 1): per-thruster efficiency and the unit change from the table's ordinate
            observer_applied  BatchEkf.update_from_solver reads the delivered thrusts in place of the commanded ones"""
        p = CurveParams.default()
        p.kind = _CURVE_KINDS[kind] if isinstance(kind, str) else int(kind)
        p.pre = _CURVE_PRES[pre] if isinstance(pre, str) else int(pre)
        p.quantum, p.k, p.kl, p.kr, p.dl, p.dr = float(quantum), float(k), float(kl), float(kr), float(dl), float(dr)
        if pre_poly is not None:
            for i, v in enumerate(_arr(pre_poly, (5,))):
                p.pre_poly[i] = float(v)
        p.observer_applied = int(bool(observer_applied))
        e = None if eff is None else np.ascontiguousarray(np.broadcast_to(np.asarray(eff, dtype=np.float64), (self.B, 6)))
        self._chk(self._L.brov_curve_set_host(self._h, C.byref(p), _dp(e)), "set_thrust_curve")

    def thrust_curve_off(self):
        """every launch as it was without the stage; the books stay readable"""
        self._chk(self._L.brov_curve_off(self._h), "thrust_curve_off")

    def thrust_curve_enabled(self):
        return bool(self._L.brov_curve_enabled(self._h))

    def thrust_curve_reset(self, stats_only=False):
        """zeroes the books and the stage's step count (stats_only: err_sq, dead_ticks, charge and the step count alone)"""
        if stats_only:
            self._chk(self._L.brov_curve_reset_stats(self._h), "thrust_curve_reset")
        else:
            self._chk(self._L.brov_curve_reset(self._h), "thrust_curve_reset")

    def thrust_curve_eval(self, values, part="both"):
        """(out [B, 6], amps [B, 6]) of the part(s) "command", "thrust" or "both" alone for `values` [B, 6]; moves nothing"""
        v = _arr(values, (self.B, 6))
        o, a = np.empty((self.B, 6)), np.empty((self.B, 6))
        pt = _CURVE_PARTS[part] if isinstance(part, str) else int(part)
        self._chk(self._L.brov_curve_eval_host(self._h, pt, _dp(v), _dp(o), _dp(a)), "thrust_curve_eval")
        return o, a

    def thrust_curve_last(self):
        """dict(u0 [B, 4], wanted [B, 6], command [B, 6], thrust [B, 6]): what the last plant step behind the stage was given and made of it"""
        u, w, c, t = np.empty((self.B, NU)), np.empty((self.B, 6)), np.empty((self.B, 6)), np.empty((self.B, 6))
        self._chk(self._L.brov_curve_last_host(self._h, _dp(u), _dp(w), _dp(c), _dp(t)), "thrust_curve_last")
        return dict(u0=u, wanted=w, command=c, thrust=t)

    def thrust_curve_stats(self):
        """dict(err_sq [B]: running sum of |wanted - delivered|^2; dead_ticks [B, 6]: steps a wanted thrust gave none; charge [B] in A s;
        steps: steps of the stage since it was set or reset)"""
        e, d, q, steps = np.empty(self.B), np.empty((self.B, 6), dtype=np.int32), np.empty(self.B), C.c_int64(0)
        self._chk(self._L.brov_curve_get_stats_host(self._h, _dp(e), d.ctypes.data_as(C.POINTER(C.c_int32)), _dp(q), C.byref(steps)),
                  "thrust_curve_stats")
        return dict(err_sq=e, dead_ticks=d, charge=q, steps=int(steps.value))

    def thrust_curve_last_seconds(self):
        """(command, thrust): duration of the last launch of either part (HIP events; one launch does both while the rotor stage is off);
        None where none was launched yet"""
        a, b = C.c_double(0.0), C.c_double(0.0)
        rc = self._L.brov_curve_last_seconds(self._h, C.byref(a), C.byref(b))
        if rc != -1:                           # (BROV_ERR_ARG: no plant step behind the stage yet)
            self._chk(rc, "thrust_curve_last_seconds")
        return (a.value, b.value) if rc == 0 else None

    # ---- ocean current on the plant: a world-frame water velocity, drag on the velocity through the water (brov_current_*) ------------------
    def set_current(self, constant=None, table=None, gain=None, gauss_markov=None):
        """the plant steps from now on run in moving water: exactly one of
            constant=      [3] for all or [B, 3], world-frame (vx, vy, vz) in m/s (current_from_angles() gives it from speed and two angles)
            table=         [rows, 3], one row per plant tick (plant_wrench_tick()), the last row repeated; gain= [B] scales it per instance
            gauss_markov=  dict(mean [3] or [B, 3], mu, amp: scalar or [3]; optional seed=0, lo=-5, hi=5: scalar or [3], step=0.05 seconds per
                           tick): per world axis c <- clamp((c - step * mu * (c - mean)) + amp * (2 U - 1), lo, hi) behind every plant step,
                           U a counter-based uniform draw of (seed, instance, tick, axis); the state starts at the mean (set_current_state())"""
        if (constant is not None) + (table is not None) + (gauss_markov is not None) != 1:
            raise ValueError("set_current takes exactly one of constant=, table=, gauss_markov=")
        if gain is not None and table is None:
            raise ValueError("gain= goes with table=")

        def rows(v, shape):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), shape))
        if constant is not None:
            self._chk(self._L.brov_current_constant_host(self._h, _dp(rows(constant, (self.B, 3)))), "set_current")
        elif table is not None:
            tab = np.ascontiguousarray(table, dtype=np.float64)
            if tab.ndim != 2 or tab.shape[1] != 3 or tab.shape[0] < 1:
                raise ValueError("current table must be [rows][3]")
            self._chk(self._L.brov_current_table_host(self._h, _dp(tab), tab.shape[0], _dp(_arr_opt(gain, (self.B,)))), "set_current")
        else:
            kw = dict(seed=0, mean=None, mu=None, amp=None, lo=None, hi=None, step=0.05)
            unknown = set(gauss_markov) - set(kw)
            if unknown:
                raise ValueError(f"unknown Gauss-Markov current parameters {sorted(unknown)}")
            kw.update(gauss_markov)
            if kw["mean"] is None or kw["mu"] is None or kw["amp"] is None:
                raise ValueError("gauss_markov= needs mean, mu and amp")
            self._chk(self._L.brov_current_gauss_markov_host(
                self._h, int(kw["seed"]) & 0xFFFFFFFFFFFFFFFF, _dp(rows(kw["mean"], (self.B, 3))), _dp(rows(kw["mu"], (3,))), _dp(rows(kw["amp"], (3,))),
                _dp(rows(kw["lo"], (3,))), _dp(rows(kw["hi"], (3,))), float(kw["step"])), "set_current")

    def current_off(self):
        """still water: the plant kernels as they always were"""
        self._chk(self._L.brov_current_off(self._h), "current_off")

    def current_mode(self):
        return int(self._L.brov_current_mode(self._h))

    def _current_out(self, fn, name, *args):
        v = np.empty((self.B, 3))
        self._chk(fn(self._h, *args, _dp(v)), name)
        return v

    def current(self, tick):
        """[B, 3]: the constant / table current of every instance at `tick`, evaluated by the device generator (moves nothing)"""
        return self._current_out(self._L.brov_current_eval_host, "current", int(tick))

    def current_state(self):
        """[B, 3]: the current the next plant step applies (Gauss-Markov mode: the state)"""
        return self._current_out(self._L.brov_current_get_state_host, "current_state")

    def set_current_state(self, v):
        """Gauss-Markov mode: the state, [3] for all or [B, 3]"""
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.B, 3)))
        self._chk(self._L.brov_current_set_state_host(self._h, _dp(v)), "set_current_state")

    def current_last(self):
        """[B, 3]: the current the last plant step applied"""
        return self._current_out(self._L.brov_current_last_host, "current_last")

    def current_last_seconds(self):
        """duration of the last plant kernel launched under a current (HIP events)"""
        sec = C.c_double(0.0)
        self._chk(self._L.brov_current_last_seconds(self._h, C.byref(sec)), "current_last_seconds")
        return sec.value

    # ---- Coriolis stage of the plant: the rigid-body and added-mass Coriolis forces the OCP model drops (brov_coriolis_*) ----------------------
    def set_coriolis(self, rigid=True, added=False, ka=0.0, ma=1.2481):
        """the plant steps from now on integrate the vehicle the reference's observer is written for: rows X, Y, Z, N of
            rigid=  -C_RB(nu) nu, the rigid-body products m (r v - q w), ...: exactly what the EKF's model has
            added=  -C_A(nu_r) nu_r of the diagonal added mass (the plant's true p[4..6] and the roll / pitch added inertia ka, ma), at the
                    velocity through the water
        evaluated afresh at every RK stage; the controller, the predictor, the observer and the estimator keep their models"""
        terms = (CORIOLIS_RIGID if rigid else 0) | (CORIOLIS_ADDED if added else 0)
        self._chk(self._L.brov_coriolis_set(self._h, terms, float(ka), float(ma)), "set_coriolis")

    def coriolis_off(self):
        """the plant kernels as they always were"""
        self._chk(self._L.brov_coriolis_off(self._h), "coriolis_off")

    def coriolis_terms(self):
        """the CORIOLIS_* bit mask in force, 0 while off"""
        return int(self._L.brov_coriolis_terms(self._h))

    def coriolis_eval(self, x, vc=None):
        """[B, 4]: the stage's force [X Y Z N] at the states x [B, 12], in water moving with the world-frame velocities vc ([3] for all or
        [B, 3]; None: still water), evaluated by the device with the plant parameters the next step would use (moves nothing)"""
        x = _arr(x, (self.B, 12))
        v = None if vc is None else np.ascontiguousarray(np.broadcast_to(np.asarray(vc, dtype=np.float64), (self.B, 3)))
        c = np.empty((self.B, 4))
        self._chk(self._L.brov_coriolis_eval_host(self._h, _dp(x), _dp(v), _dp(c)), "coriolis_eval")
        return c

    def coriolis_last(self):
        """[B, 4]: the stage's force at the start state of the last plant step under it"""
        c = np.empty((self.B, 4))
        self._chk(self._L.brov_coriolis_last_host(self._h, _dp(c)), "coriolis_last")
        return c

    def coriolis_last_seconds(self):
        """duration of the last plant kernel launched under the Coriolis stage (HIP events)"""
        sec = C.c_double(0.0)
        self._chk(self._L.brov_coriolis_last_seconds(self._h, C.byref(sec)), "coriolis_last_seconds")
        return sec.value

    # ---- sensor stage between plant and controller: noise, bias, quantisation, slow and dropped fixes (brov_sensor_*) ------------------
    def set_sensors(self, seed=0, sigma=None, bias=None, quant=None, period=None, dropout=None):
        """from now on solve(), the loops, the observer and the estimator read the MEASURED state instead of the plant's true state (the plant,
        the logs and the tracker keep the true one); the statistics start afresh and the measured state is refreshed from x0.  The fresh sample
        of channel c at measurement index m (plant_wrench_tick()): v = (x + bias) + sigma * n(b, m, c);  y = rint(v / quant) * quant where
        quant > 0.  n is an Irwin-Hall(12) variate -- unit variance, bounded by +-6, kurtosis 2.9 --, not a Gaussian.
            sigma, bias  scalar, [12] or [B, 12] (None: 0)
            quant        scalar or [12], shared by the batch (None or 0: none)
            period       scalar or [12] int >= 1: a plant step refreshes channel c where the index is a multiple of period[c] (None: 1)
            dropout      scalar or [B] in [0, 1]: probability that the fix behind a plant step is dropped and every channel holds (None: 0)"""
        def rows(v, shape, dtype=np.float64):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), shape))
        sg, bi, dr = rows(sigma, (self.B, NX)), rows(bias, (self.B, NX)), rows(dropout, (self.B,))
        qu, pe = rows(quant, (NX,)), rows(period, (NX,), np.int32)
        self._chk(self._L.brov_sensor_set_host(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, _dp(sg), _dp(bi), _dp(qu),
                                               None if pe is None else pe.ctypes.data_as(C.POINTER(C.c_int32)), _dp(dr)), "set_sensors")

    def sensors_off(self):
        """everything reads the plant's true state again, no extra launch; the statistics stay readable"""
        self._chk(self._L.brov_sensor_off(self._h), "sensors_off")

    def sensors_enabled(self):
        return bool(self._L.brov_sensor_enabled(self._h))

    def sensor_measure(self, stream=0):
        """a forced refresh of the measured state at the current index, for a caller that wrote x0 through x0_device_ptr()"""
        self._chk(self._L.brov_sensor_measure(self._h, C.c_void_p(stream)), "sensor_measure")

    def sensor_eval(self, index, x):
        """(y [B, 12], dropped [B] int32): fresh samples of the states `x` [B, 12] at `index` and the dropout verdicts of that index; moves
        nothing, touches no statistic"""
        xa = _arr(x, (self.B, NX))
        y, dr = np.empty((self.B, NX)), np.zeros(self.B, dtype=np.int32)
        self._chk(self._L.brov_sensor_eval_host(self._h, int(index), _dp(xa), _dp(y), dr.ctypes.data_as(C.POINTER(C.c_int32))), "sensor_eval")
        return y, dr

    def measured_state(self):
        """[B, 12]: the measured state as the last refresh left it"""
        y = np.empty((self.B, NX))
        self._chk(self._L.brov_sensor_get_measurement_host(self._h, _dp(y)), "measured_state")
        return y

    def sensor_stats(self):
        """dict(dropped [B] int32: fixes dropped; err_sq [B, 12]: running sum of (measured - true)^2 behind every plant step, held values
        included; refreshes: plant steps behind which the stage ran since the statistics were reset)"""
        dr, esq, n = np.zeros(self.B, dtype=np.int32), np.empty((self.B, NX)), C.c_int64(0)
        self._chk(self._L.brov_sensor_get_stats_host(self._h, dr.ctypes.data_as(C.POINTER(C.c_int32)), _dp(esq), C.byref(n)), "sensor_stats")
        return dict(dropped=dr, err_sq=esq, refreshes=int(n.value))

    def sensor_reset_stats(self):
        self._chk(self._L.brov_sensor_reset_stats(self._h), "sensor_reset_stats")

    def sensor_last_seconds(self):
        """duration of the measure kernel's last launch (HIP events)"""
        sec = C.c_double(0.0)
        self._chk(self._L.brov_sensor_last_seconds(self._h, C.byref(sec)), "sensor_last_seconds")
        return sec.value

    # ---- IMU/GPS stage behind the plant: what the error-state filter reads, at the sensors' own rates (brov_imu_*) ----------------------
    def set_imu(self, h, gps_every=1, seed=0, sigma=None, bias=None, dropout=None, g=9.81, flags=0):
        """from now on every plant step (whose dt must be exactly h) is followed by a sample of the IMU/GPS stage from the TRUE state: the
        mean specific force of the step and the body rates, and, where the index is a multiple of gps_every and the fix is not dropped, a
        position fix, its differenced velocity and an attitude (include/bluerov2_nmpc_imu.h has the formulas).  The stage restarts.
            sigma    scalar, [12] or [B, 12]: accelerometer, gyro, GPS position, attitude (None: 0)
            bias     scalar, [6] or [B, 6]: accelerometer, gyro (None: 0)
            dropout  scalar or [B] in [0, 1]: probability that a due fix is dropped (None: 0)
            flags    IMU_GPSV_ELAPSED: gps_v divides by the time since the last fix taken, not by the nominal period"""
        def rows(v, shape):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), shape))
        par = ImuParams(float(h), float(g), int(gps_every), int(flags), int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._chk(self._L.brov_imu_set_host(self._h, C.byref(par), _dp(rows(sigma, (self.B, 12))), _dp(rows(bias, (self.B, 6))),
                                            _dp(rows(dropout, (self.B,)))), "set_imu")

    def imu_off(self):
        """no launch behind a plant step any more; the statistics stay readable"""
        self._chk(self._L.brov_imu_off(self._h), "imu_off")

    def imu_enabled(self):
        return bool(self._L.brov_imu_enabled(self._h))

    def imu_restart(self, stream=0):
        """a forced restart at the current index: the acceleration is gravity alone, a fix is taken with gps_v = 0"""
        self._chk(self._L.brov_imu_restart(self._h, C.c_void_p(stream)), "imu_restart")

    def imu_eval(self, index, x, v_prev, gps_p_last, m_last):
        """dict(imu [B, 6], gps_p [B, 3], gps_v [B, 3], q_meas [B, 4], fix [B] int32): the stage alone at `index` for the states `x` [B, 12],
        the previous inertial velocity [B, 3], the last fix [B, 3] and its index [B] (< 0: none); without a fix the last three are zeros.
        Moves nothing, touches no statistic"""
        ml = _arr(m_last, (self.B,), np.int32)
        o = dict(imu=np.empty((self.B, 6)), gps_p=np.empty((self.B, 3)), gps_v=np.empty((self.B, 3)), q_meas=np.empty((self.B, 4)),
                 fix=np.zeros(self.B, dtype=np.int32))
        ip = C.POINTER(C.c_int32)
        self._chk(self._L.brov_imu_eval_host(self._h, int(index), _dp(_arr(x, (self.B, NX))), _dp(_arr(v_prev, (self.B, 3))),
                                             _dp(_arr(gps_p_last, (self.B, 3))), ml.ctypes.data_as(ip), _dp(o["imu"]), _dp(o["gps_p"]),
                                             _dp(o["gps_v"]), _dp(o["q_meas"]), o["fix"].ctypes.data_as(ip)), "imu_eval")
        return o

    def imu(self):
        """dict(imu, gps_p, gps_v, q_meas, fix): the last sample and its flags as the stage holds them"""
        o = dict(imu=np.empty((self.B, 6)), gps_p=np.empty((self.B, 3)), gps_v=np.empty((self.B, 3)), q_meas=np.empty((self.B, 4)),
                 fix=np.zeros(self.B, dtype=np.int32))
        self._chk(self._L.brov_imu_get_host(self._h, _dp(o["imu"]), _dp(o["gps_p"]), _dp(o["gps_v"]), _dp(o["q_meas"]),
                                            o["fix"].ctypes.data_as(C.POINTER(C.c_int32))), "imu")
        return o

    def imu_stats(self):
        """dict(samples, fixes, dropped: [B] int32 each, of the regular refreshes; refreshes: plant steps behind which the stage ran)"""
        st, n = np.zeros((self.B, 3), dtype=np.int32), C.c_int64(0)
        self._chk(self._L.brov_imu_get_stats_host(self._h, st.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)), "imu_stats")
        return dict(samples=st[:, 0].copy(), fixes=st[:, 1].copy(), dropped=st[:, 2].copy(), refreshes=int(n.value))

    def imu_reset_stats(self):
        self._chk(self._L.brov_imu_reset_stats(self._h), "imu_reset_stats")

    def imu_last_seconds(self):
        """duration of the stage's last refresh (HIP events)"""
        sec = C.c_double(0.0)
        self._chk(self._L.brov_imu_last_seconds(self._h, C.byref(sec)), "imu_last_seconds")
        return sec.value

    # ---- range stage and inspection controller: the reference's bridge demo (brov_range_*, brov_inspect_*) ---------------------------------
    def set_range_scene(self, lo, hi):
        """the scene of the range stage: n <= RANGE_MAX_BOXES axis-aligned world-frame boxes, lo and hi [n, 3], shared by the batch"""
        lo, hi = np.ascontiguousarray(lo, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(hi, dtype=np.float64).reshape(-1, 3)
        if lo.shape != hi.shape:
            raise ValueError("lo and hi must have the same shape [n, 3]")
        self._chk(self._L.brov_range_set_scene_host(self._h, len(lo), _dp(lo), _dp(hi)), "set_range_scene")

    def set_range(self, params=None, sigma=None, **kw):
        """the camera (RangeParams; None: the defaults, with the fields given as keywords changed; mount=(x, y, z)) and the standard deviation
        of the range noise, a scalar or [B] (None: 0)"""
        p = params if params is not None else _inspect.default_range_params()
        for k, v in kw.items():
            if k == "mount":
                p.mount[:] = [float(a) for a in v]
            else:
                setattr(p, k, v)
        sg = None if sigma is None else np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (self.B,)))
        self._chk(self._L.brov_range_set_host(self._h, C.byref(p), _dp(sg)), "set_range")
        self._roi = int(p.roi)

    def set_range_mesh(self, tri, leaf=0):
        """the triangle mesh of the range stage's scene, beside the boxes: tri [T, 3, 3] world-frame vertices (mesh.load_stl reads a binary
        STL file), shared by the batch; leaf: the largest number of triangles in a leaf of the hierarchy, 1 ... 8 (0: 4), which changes no
        result.  None or an empty array removes the mesh"""
        t = np.zeros((0, 3, 3)) if tri is None else np.ascontiguousarray(tri, dtype=np.float64)
        if t.ndim != 3 or t.shape[1:] != (3, 3):
            raise ValueError("tri must have the shape [T, 3, 3]")
        self._chk(self._L.brov_mesh_set_host(self._h, len(t), _dp(t) if len(t) else None, int(leaf)), "set_range_mesh")

    def range_mesh_info(self):
        """MeshInfo: triangles, nodes, leaves, depth, device bytes and pad of the mesh in force (zeros: none)"""
        info = MeshInfo()
        self._chk(self._L.brov_mesh_info(self._h, C.byref(info)), "range_mesh_info")
        return info

    def range_eval(self, index, x, rot=False, depth=False, visits=False):
        """dict(range [B], hits [B] int32, and with rot / depth: rot [B, 9], depth [B, roi * roi] with 0.0 where a ray has no return): the
        range stage alone at `index` for the states `x` [B, 12].  Moves nothing.  visits (needs a mesh): visits [B, 2] int64, the node tests
        and triangle tests the rays of each instance made"""
        roi = getattr(self, "_roi", 40)
        o = dict(range=np.empty(self.B), hits=np.zeros(self.B, dtype=np.int32))
        if rot:
            o["rot"] = np.empty((self.B, 9))
        if depth:
            o["depth"] = np.empty((self.B, roi * roi))
        if visits:
            o["visits"] = np.zeros((self.B, 2), dtype=np.int64)
            self._chk(self._L.brov_mesh_eval_host(self._h, int(index), _dp(_arr(x, (self.B, NX))), _dp(o["range"]),
                                                  o["hits"].ctypes.data_as(C.POINTER(C.c_int32)), _dp(o.get("rot")), _dp(o.get("depth")),
                                                  o["visits"].ctypes.data_as(C.POINTER(C.c_int64))), "range_eval")
            return o
        self._chk(self._L.brov_range_eval_host(self._h, int(index), _dp(_arr(x, (self.B, NX))), _dp(o["range"]),
                                               o["hits"].ctypes.data_as(C.POINTER(C.c_int32)), _dp(o.get("rot")), _dp(o.get("depth"))), "range_eval")
        return o

    def range_last_seconds(self):
        sec = C.c_double(0.0)
        self._chk(self._L.brov_range_last_seconds(self._h, C.byref(sec)), "range_last_seconds")
        return sec.value

    def set_inspect(self, params=None, **kw):
        """the inspection controller comes into force with a fresh state and statistics (InspectParams; None: the node's values, with the
        fields given as keywords changed; gains=[9]).  From now on inspect_step writes the records a solve would write"""
        p = params if params is not None else _inspect.default_inspect_params()
        for k, v in kw.items():
            if k == "gains":
                p.gains[:] = [float(a) for a in v]
            else:
                setattr(p, k, v)
        self._chk(self._L.brov_inspect_set_host(self._h, C.byref(p)), "set_inspect")

    def inspect_off(self):
        self._chk(self._L.brov_inspect_off(self._h), "inspect_off")

    def inspect_enabled(self):
        return bool(self._L.brov_inspect_enabled(self._h))

    def inspect_reset(self):
        """the state of the node's constructor, k = 0; the statistics stay"""
        self._chk(self._L.brov_inspect_reset(self._h), "inspect_reset")

    def inspect_eval(self, state, range_, z, psi, stats=None):
        """(state_out [B] of INSPECT_STATE_DTYPE, records [B] of RESULT_DTYPE, stats_out or None): the controller alone, one tick from
        `state` on the given range, z and psi [B] with the parameters in force; `stats` [B] of INSPECT_STATS_DTYPE moves along.  Moves nothing"""
        si = _arr(state, (self.B,), INSPECT_STATE_DTYPE)
        so, rec = np.zeros(self.B, dtype=INSPECT_STATE_DTYPE), np.zeros(self.B, dtype=RESULT_DTYPE)
        st = None if stats is None else _arr(stats, (self.B,), INSPECT_STATS_DTYPE).copy()
        self._chk(self._L.brov_inspect_eval_host(self._h, C.c_void_p(si.ctypes.data), _dp(_arr(range_, (self.B,))), _dp(_arr(z, (self.B,))),
                                                 _dp(_arr(psi, (self.B,))), C.c_void_p(so.ctypes.data), C.c_void_p(rec.ctypes.data),
                                                 None if st is None else C.c_void_p(st.ctypes.data)), "inspect_eval")
        return so, rec, st

    def inspect_state(self):
        """(state [B] of INSPECT_STATE_DTYPE, the last range [B])"""
        s, r = np.zeros(self.B, dtype=INSPECT_STATE_DTYPE), np.empty(self.B)
        self._chk(self._L.brov_inspect_get_state_host(self._h, C.c_void_p(s.ctypes.data), _dp(r)), "inspect_state")
        return s, r

    def inspect_stats(self):
        """[B] of INSPECT_STATS_DTYPE: ticks per status, rounds, visits of the "failed" branch, first tick with the mission completed,
        the sum of (range - safety_dis)^2 over the status-0 ticks, the smallest non-zero range"""
        t = np.zeros(self.B, dtype=INSPECT_STATS_DTYPE)
        self._chk(self._L.brov_inspect_get_stats_host(self._h, C.c_void_p(t.ctypes.data)), "inspect_stats")
        return t

    def inspect_reset_stats(self):
        self._chk(self._L.brov_inspect_reset_stats(self._h), "inspect_reset_stats")

    def inspect_last_seconds(self):
        sec = C.c_double(0.0)
        self._chk(self._L.brov_inspect_last_seconds(self._h, C.byref(sec)), "inspect_last_seconds")
        return sec.value

    def inspect_step(self, stream=0):
        """one tick of the controller: rays from the true state at the plant's tick counter, then the record into results()"""
        self._chk(self._L.brov_inspect_step(self._h, C.c_void_p(stream)), "inspect_step")

    def closed_loop_inspect(self, ticks, dt=0.05, substeps=1, log=True):
        """ticks x (inspect_step -> plant_step) on the device, one host wait; returns (u_log [ticks, B, 4], x_log [ticks + 1, B, 12],
        status_log [ticks, B] the mission status, range_log [ticks, B]) or None"""
        if not log:
            self._chk(self._L.brov_closed_loop_inspect(self._h, int(ticks), float(dt), int(substeps), None, None, None, None), "closed_loop_inspect")
            return None
        ul, xl = np.empty((ticks, self.B, NU)), np.empty((ticks + 1, self.B, NX))
        sl, rl = np.empty((ticks, self.B), dtype=np.int32), np.empty((ticks, self.B))
        self._chk(self._L.brov_closed_loop_inspect(self._h, int(ticks), float(dt), int(substeps), _dp(ul), _dp(xl),
                                                   sl.ctypes.data_as(C.POINTER(C.c_int32)), _dp(rl)), "closed_loop_inspect")
        return ul, xl, sl, rl

    # ---- iterate ----------------------------------------------------------------------------------------------
    def set_iterate(self, x=None, u=None, pi=None, lam=None):
        B, N = self.B, self.N
        ax, au = _arr_opt(x, (B, N + 1, NX)), _arr_opt(u, (B, N, NU))
        ap, al = _arr_opt(pi, (B, N, NX)), _arr_opt(lam, (B, N, 8))
        self._chk(self._L.brov_set_iterate_host(self._h, _dp(ax), _dp(au), _dp(ap), _dp(al)), "set_iterate")

    def get_iterate(self):
        B, N = self.B, self.N
        x, u = np.empty((B, N + 1, NX)), np.empty((B, N, NU))
        pi, lam = np.empty((B, N, NX)), np.empty((B, N, 8))
        self._chk(self._L.brov_get_iterate_host(self._h, _dp(x), _dp(u), _dp(pi), _dp(lam)), "get_iterate")
        return x, u, pi, lam

    def reset(self):
        self._chk(self._L.brov_reset(self._h), "reset")

    def init_iterate_default(self):
        self._chk(self._L.brov_init_iterate_default(self._h), "init_iterate_default")

    # ---- solve / outputs --------------------------------------------------------------------------------------
    def solve(self, stream=0, sync=False):
        self._chk(self._L.brov_solve(self._h, C.c_void_p(stream)), "solve")
        if sync:
            self._chk(self._L.brov_synchronize(self._h, C.c_void_p(stream)), "synchronize")

    def results(self):
        res = np.zeros(self.B, dtype=RESULT_DTYPE)
        self._chk(self._L.brov_get_results_host(self._h, C.c_void_p(res.ctypes.data)), "results")
        return res

    def u0(self):
        u0 = np.empty((self.B, NU))
        self._chk(self._L.brov_get_u0_host(self._h, _dp(u0)), "u0")
        return u0

    def thrusts(self):
        t = np.empty((self.B, 6))
        self._chk(self._L.brov_get_thrusts_host(self._h, _dp(t)), "thrusts")
        return t

    def debug_dump_linearisation(self, on=True):
        """make the LDS-resident kernels write their [A B | b] out so that linearisation() works for them too (tests)"""
        self._chk(self._L.brov_debug_dump_linearisation(self._h, int(on)), "debug_dump_linearisation")

    def linearisation(self):
        AB, b = np.empty((self.B, self.N, NX, 16)), np.empty((self.B, self.N, NX))
        self._chk(self._L.brov_get_linearisation_host(self._h, _dp(AB), _dp(b)), "linearisation")
        return AB[..., :NX], AB[..., NX:], b

    def select_best(self):
        idx = C.c_int(-1)
        rec = np.zeros(1, dtype=RESULT_DTYPE)
        self._chk(self._L.brov_select_best_host(self._h, C.byref(idx), C.c_void_p(rec.ctypes.data)), "select_best")
        return idx.value, rec[0]

    def enable_timing(self, on=True):
        self._chk(self._L.brov_enable_timing(self._h, int(on)), "enable_timing")

    def last_kernel_path(self):
        return int(self._L.brov_last_kernel_path(self._h))

    def window_stages(self):
        """stages per LDS window of the windowed kernel (0: none; == N: resident mode, the whole horizon in one window)"""
        return int(self._L.brov_window_stages(self._h))

    def lds_kernel_info(self):
        """dict(lds_bytes_per_block, blocks_per_cu, threads_per_block, kind) of the LDS-resident kernel this solver launches"""
        a = (C.c_int32 * 4)()
        self._chk(self._L.brov_lds_kernel_info(self._h, a), "lds_kernel_info")
        kind = {0: "streaming", 1: "fused", 2: "fused, two waves per SIMD", 3: "windowed", 4: "windowed, resident"}[int(a[3])]
        return dict(lds_bytes_per_block=int(a[0]), blocks_per_cu=int(a[1]), threads_per_block=int(a[2]), kind=kind)

    def last_solve_seconds(self):
        tot, k2 = C.c_double(0), (C.c_double * 2)()
        self._chk(self._L.brov_last_solve_seconds(self._h, C.byref(tot), k2), "last_solve_seconds")
        return tot.value, (k2[0], k2[1])

    # device pointers for zero-copy pipelines
    def results_device_ptr(self):
        return int(self._L.brov_results_device(self._h))

    def x0_device_ptr(self):
        return int(self._L.brov_x0_device(self._h))


def selftest_sweep12(a):
    """inverse of an SPD 12 x 12 matrix by the parallel-in-time kernel's block sweeps: (inverse, all pivot blocks positive definite)"""
    L = _load()
    a = _arr(a, (12, 12))
    out, ok = np.empty((12, 12)), C.c_int(0)
    rc = L.brov_selftest_sweep12(_dp(a), _dp(out), C.byref(ok))
    if rc == -2:
        raise NoDeviceError("no HIP device")
    if rc != 0:
        raise RuntimeError(f"selftest failed {rc}")
    return out, bool(ok.value)


def selftest_tile_tn(xt, y, c, k4):
    L = _load()
    xt, y, c = _arr(xt, (16, 16)), _arr(y, (16, 16)), _arr(c, (16, 16))
    out = np.empty((16, 16))
    rc = L.brov_selftest_tile_tn(_dp(xt), _dp(y), _dp(c), _dp(out), int(k4))
    if rc == -2:
        raise NoDeviceError("no HIP device")
    if rc != 0:
        raise RuntimeError(f"selftest failed {rc}")
    return out


def selftest_model(a=None, d=None, x=None, u=None, p=None, ww=None, rp=None):
    """the device model's building blocks alone, one lane per item (csrc/model_selftest.hip): sincos_pio2(a[n]), rcp_nr(d[n]) and
    model_f of x[n,12], u[n,4], p[n,16] without and with the world wrench ww[n,6], both with the roll / pitch moments rp[n,2].
    Arguments left out are filled with harmless values.  Returns dict(sin, cos, rcp [n], f, f_ww [n,12])."""
    L = _load()
    given = [v for v in (a, d, x, u, p, ww, rp) if v is not None]
    if not given:
        raise ValueError("selftest_model needs at least one input array")
    n = len(given[0])

    def arg(v, cols, fill):
        if v is None:
            return np.full((n, cols) if cols else (n,), fill, dtype=np.float64)
        return _arr(v, (n, cols) if cols else (n,))
    a, d = arg(a, 0, 0.0), arg(d, 0, 1.0)
    rows = np.ascontiguousarray(np.concatenate([arg(x, NX, 0.0), arg(u, NU, 0.0), arg(p, NP, 0.0), arg(ww, 6, 0.0), arg(rp, 2, 0.0)], axis=1))
    out = np.empty((n, 27))
    rc = L.brov_selftest_model(_dp(a), _dp(d), _dp(rows), _dp(out), n)
    if rc == -2:
        raise NoDeviceError("no HIP device")
    if rc != 0:
        raise RuntimeError(f"selftest failed {rc}")
    return dict(sin=out[:, 0].copy(), cos=out[:, 1].copy(), rcp=out[:, 2].copy(), f=out[:, 3:15].copy(), f_ww=out[:, 15:27].copy())
