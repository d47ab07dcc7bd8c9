"""Host-side mirror of the batched error-state Kalman filter with IMU disturbance observer (include/bluerov2_nmpc_eskf.h, brov_eskf_*;
reference: the bluerov2_states nodelet, src/Eskf.cpp).  ctypes over the HIP library -- no CPU path."""
import ctypes as C

import numpy as np

from .solver import _Handle, _arr, _arr_opt, _bind, _dp, _load, BatchSolver


class EskfParams(C.Structure):
    """brov_eskf_params; defaults via EskfParams.default() = the reference's constants (ImuDo.h:101-110, Config.cpp, launch/config/imudo.yaml)"""
    _fields_ = [("dt", C.c_double), ("gps_dt", C.c_double), ("mass", C.c_double), ("ZG", C.c_double), ("g", C.c_double), ("bouyancy", C.c_double),
                ("added_mass", C.c_double * 6), ("Dl", C.c_double * 6), ("Dnl", C.c_double * 6), ("K", C.c_double * 36), ("Q", C.c_double * 21),
                ("R12", C.c_double * 12), ("vel_inject", C.c_double), ("compensate_coef", C.c_double), ("rotor_constant", C.c_double),
                ("inject_bias_g", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def default(cls):
        p = cls()
        _eskf_lib().brov_eskf_default_params(C.byref(p))
        return p


def _protos(L):
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.brov_eskf_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(EskfParams)]
    _bind(L, {"brov_eskf_last_error": []}, C.c_char_p)
    _bind(L, {"brov_eskf_default_params": [C.POINTER(EskfParams)], "brov_eskf_destroy": [vp]}, None)
    _bind(L, {"brov_eskf_x_device": [vp], "brov_eskf_P_device": [vp], "brov_eskf_mpc_p_device": [vp]}, vp)
    _bind(L, {
        "brov_eskf_batch": [vp], "brov_eskf_reset": [vp, dp, dp], "brov_eskf_set_state_host": [vp, dp, dp],
        "brov_eskf_get_state_host": [vp, dp, dp], "brov_eskf_predict_host": [vp, dp, vp], "brov_eskf_predict_device": [vp, vp, vp],
        "brov_eskf_update_host": [vp, dp, dp, dp, dp, dp, vp], "brov_eskf_update_device": [vp, vp, vp, vp, vp, vp, vp],
        "brov_eskf_get_outputs_host": [vp, dp, dp, dp, ip], "brov_eskf_get_inputs_host": [vp, dp, dp, dp, dp, dp],
        "brov_eskf_update_from_solver": [vp, vp, vp], "brov_eskf_apply_to_solver": [vp, vp, vp],
        "brov_eskf_last_update_seconds": [vp, dp],
        "brov_imu_eskf_tick_host": [vp, dp, dp, dp, dp, dp, ip, vp], "brov_imu_eskf_tick_device": [vp, vp, vp, vp, vp, vp, vp, vp],
        "brov_imu_eskf_tick_from_solver": [vp, vp, vp],
    })
    _bind(L, {"brov_imu_eskf_xi_world_device": [vp]}, vp)
    L.brov_closed_loop_eskf.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, ip, dp, dp, ip]
    L.brov_closed_loop_eskf.restype = C.c_int


def _eskf_lib():
    return _load(_protos)


class BatchEskf(_Handle):
    """B independent 21-state error-state filters resident on one GPU; predict() = a tick without a GPS fix, update() = predict followed by update."""
    _last_error, _destroy = "brov_eskf_last_error", "brov_eskf_destroy"

    def __init__(self, batch, params=None, device=0):
        L = _eskf_lib()
        self.B = int(batch)
        self.params = params if params is not None else EskfParams.default()
        self._create(L, "brov_eskf_create", int(device), self.B, C.byref(self.params))

    def reset(self, x0=None, P0=None):
        self._chk(self._L.brov_eskf_reset(self._h, _dp(_arr_opt(x0, (22,))), _dp(_arr_opt(P0, (21, 21)))), "reset")

    def set_state(self, x=None, P=None):
        self._chk(self._L.brov_eskf_set_state_host(self._h, _dp(_arr_opt(x, (self.B, 22))), _dp(_arr_opt(P, (self.B, 21, 21)))), "set_state")

    def state(self):
        x = np.empty((self.B, 22)); P = np.empty((self.B, 21, 21))
        self._chk(self._L.brov_eskf_get_state_host(self._h, _dp(x), _dp(P)), "get_state")
        return x, P

    def predict(self, imu, stream=0):
        self._chk(self._L.brov_eskf_predict_host(self._h, _dp(_arr(imu, (self.B, 6))), C.c_void_p(stream)), "predict")

    def predict_device(self, imu_ptr, stream=0):
        self._chk(self._L.brov_eskf_predict_device(self._h, C.c_void_p(imu_ptr), C.c_void_p(stream)), "predict_device")

    def update(self, imu, gps_p, gps_v, q_meas, thrust, stream=0):
        imu = _arr(imu, (self.B, 6)); gps_p = _arr(gps_p, (self.B, 3)); gps_v = _arr(gps_v, (self.B, 3))
        q_meas = _arr(q_meas, (self.B, 4)); thrust = _arr(thrust, (self.B, 6))
        self._chk(self._L.brov_eskf_update_host(self._h, _dp(imu), _dp(gps_p), _dp(gps_v), _dp(q_meas), _dp(thrust), C.c_void_p(stream)), "update")

    def update_device(self, imu_ptr, gps_p_ptr, gps_v_ptr, q_meas_ptr, thrust_ptr, stream=0):
        self._chk(self._L.brov_eskf_update_device(self._h, *(C.c_void_p(p) for p in (imu_ptr, gps_p_ptr, gps_v_ptr, q_meas_ptr, thrust_ptr)),
                                                  C.c_void_p(stream)), "update_device")

    def outputs(self):
        """(body-frame disturbance xi [B,3], xi_world [B,3], NMPC parameters p[0..3] [B,4], status [B])"""
        xi = np.empty((self.B, 3)); xw = np.empty((self.B, 3)); mp = np.empty((self.B, 4)); st = np.empty(self.B, dtype=np.int32)
        self._chk(self._L.brov_eskf_get_outputs_host(self._h, _dp(xi), _dp(xw), _dp(mp), st.ctypes.data_as(C.POINTER(C.c_int32))), "outputs")
        return xi, xw, mp, st

    def inputs(self):
        """(imu [B,6], gps_p [B,3], gps_v [B,3], q_meas [B,4], thrust [B,6]) of the last update tick, as the observer holds them"""
        out = tuple(np.empty((self.B, n)) for n in (6, 3, 3, 4, 6))
        self._chk(self._L.brov_eskf_get_inputs_host(self._h, *(_dp(a) for a in out)), "inputs")
        return out

    def tick(self, imu, gps_p, gps_v, q_meas, thrust, fix, stream=0):
        """one launch for the batch: filter b does the update tick where fix[b] != 0 and the predict-only tick where it is 0, bit for bit;
        what a filter without a fix has in gps_p, gps_v, q_meas and thrust reaches nothing"""
        imu = _arr(imu, (self.B, 6)); gps_p = _arr(gps_p, (self.B, 3)); gps_v = _arr(gps_v, (self.B, 3))
        q_meas = _arr(q_meas, (self.B, 4)); thrust = _arr(thrust, (self.B, 6)); fix = _arr(fix, (self.B,), np.int32)
        self._chk(self._L.brov_imu_eskf_tick_host(self._h, _dp(imu), _dp(gps_p), _dp(gps_v), _dp(q_meas), _dp(thrust),
                                              fix.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream)), "tick")

    def tick_device(self, imu_ptr, gps_p_ptr, gps_v_ptr, q_meas_ptr, thrust_ptr, fix_ptr, stream=0):
        self._chk(self._L.brov_imu_eskf_tick_device(self._h, *(C.c_void_p(p) for p in (imu_ptr, gps_p_ptr, gps_v_ptr, q_meas_ptr, thrust_ptr, fix_ptr)),
                                                C.c_void_p(stream)), "tick_device")

    def tick_from_solver(self, solver: BatchSolver, stream=0):
        """the tick at the sensors' rates: the last sample of the solver's IMU/GPS stage (solver.set_imu) and its fix flags"""
        self._chk(self._L.brov_imu_eskf_tick_from_solver(self._h, solver._h, C.c_void_p(stream)), "tick_from_solver")

    def update_from_solver(self, solver: BatchSolver, stream=0):
        self._chk(self._L.brov_eskf_update_from_solver(self._h, solver._h, C.c_void_p(stream)), "update_from_solver")

    def apply_to_solver(self, solver: BatchSolver, stream=0):
        self._chk(self._L.brov_eskf_apply_to_solver(self._h, solver._h, C.c_void_p(stream)), "apply_to_solver")

    def last_update_seconds(self):
        s = C.c_double()
        self._chk(self._L.brov_eskf_last_update_seconds(self._h, C.byref(s)), "last_update_seconds")
        return s.value


def closed_loop_eskf(solver: BatchSolver, eskf: BatchEskf, ticks, line0=0, ncols=16, dt=0.05, imu_per_tick=1, log=True):
    """the control loop with the filter at its sensors' rates on the device (brov_closed_loop_eskf): ticks x (window -> RTI step ->
    imu_per_tick x (plant step of dt / imu_per_tick -> tick_from_solver) -> apply_to_solver), one host wait.  Returns dict(u, x, status,
    wrench, est [ticks, B, 3]: xi_world after each tick, fix [ticks, imu_per_tick, B]) or None"""
    L, B = _eskf_lib(), solver.B
    args = (solver._h, eskf._h, int(ticks), int(line0), int(ncols), float(dt), int(imu_per_tick))
    if not log:
        solver._chk(L.brov_closed_loop_eskf(*args, None, None, None, None, None, None), "closed_loop_eskf")
        return None
    ip = C.POINTER(C.c_int32)
    ul, xl, sl = np.empty((ticks, B, 4)), np.empty((ticks + 1, B, 12)), np.empty((ticks, B), dtype=np.int32)
    wl, el, fl = np.empty((ticks, B, 6)), np.empty((ticks, B, 3)), np.empty((ticks, int(imu_per_tick), B), dtype=np.int32)
    solver._chk(L.brov_closed_loop_eskf(*args, _dp(ul), _dp(xl), sl.ctypes.data_as(ip), _dp(wl), _dp(el), fl.ctypes.data_as(ip)),
                "closed_loop_eskf")
    return dict(u=ul, x=xl, status=sl, wrench=wl, est=el, fix=fl)
