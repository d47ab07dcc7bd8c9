"""Host-side mirror of the batched RLS-FF parameter estimator (include/bluerov2_nmpc.h, brov_rls_*; reference:
BLUEROV2_AMPC::RLSFF, bluerov2_dobmpc/src/bluerov2_ampc.cpp:731-1046).  ctypes over the HIP library -- no CPU path."""
import ctypes as C

import numpy as np

from .solver import _Handle, _arr, _arr_opt, _bind, _dp, _load, BatchSolver

APPLY_DISTURBANCE = 0   # BROV_RLS_APPLY_DISTURBANCE: p[0..3] (the shipped AMPC)
APPLY_MODEL = 1         # BROV_RLS_APPLY_MODEL: also p[4..15] from theta(0), theta(1), theta(3)


class RlsParams(C.Structure):
    """brov_rls_params; defaults via RlsParams.default() = the reference's constants (bluerov2_ampc.h:171-180,239-240)"""
    _fields_ = [("n_short", C.c_int32), ("n_long", C.c_int32), ("threshold", C.c_double), ("lambda_step", C.c_double),
                ("lambda_min", C.c_double), ("lambda_max", C.c_double), ("lambda0", C.c_double), ("p0", C.c_double),
                ("dt", C.c_double), ("compensate_coef", C.c_double), ("rotor_constant", C.c_double)]

    @classmethod
    def default(cls):
        p = cls()
        _rls_lib().brov_rls_default_params(C.byref(p))
        return p


def _protos(L):
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.brov_rls_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(RlsParams)]
    _bind(L, {"brov_rls_last_error": []}, C.c_char_p)
    _bind(L, {"brov_rls_default_params": [C.POINTER(RlsParams)], "brov_rls_destroy": [vp]}, None)
    _bind(L, {"brov_rls_theta_device": [vp]}, vp)
    _bind(L, {
        "brov_rls_batch": [vp], "brov_rls_reset": [vp], "brov_rls_set_state_host": [vp, dp, dp, dp],
        "brov_rls_get_state_host": [vp, dp, dp, dp, dp, dp], "brov_rls_update_host": [vp, dp, dp, dp, dp, vp],
        "brov_rls_update_device": [vp, vp, vp, vp, vp, vp], "brov_rls_update_from_ekf": [vp, vp, vp, vp],
        "brov_rls_apply_to_solver": [vp, vp, C.c_int, vp], "brov_rls_get_outputs_host": [vp, dp, dp, ip],
        "brov_rls_last_update_seconds": [vp, dp],
    })


def _rls_lib():
    return _load(_protos)


class BatchRls(_Handle):
    """B independent four-axis RLS-FF estimators resident on one GPU; update() = one RLSFF() tick of each.
    Axis order X, Y, Z, N; theta [B, 4 axes, 4], P [B, 4, 4, 4], lambda / F / e [B, 4]."""
    _last_error, _destroy = "brov_rls_last_error", "brov_rls_destroy"

    def __init__(self, batch, params=None, device=0):
        L = _rls_lib()
        self.B = int(batch)
        self.params = params if params is not None else RlsParams.default()
        self._create(L, "brov_rls_create", int(device), self.B, C.byref(self.params))

    def reset(self):
        self._chk(self._L.brov_rls_reset(self._h), "reset")

    def set_state(self, theta=None, P=None, lam=None):
        """any of theta [B,4,4], P [B,4,4,4], lambda [B,4]; the error windows are emptied"""
        theta = _arr_opt(theta, (self.B, 4, 4)); P = _arr_opt(P, (self.B, 4, 4, 4)); lam = _arr_opt(lam, (self.B, 4))
        self._chk(self._L.brov_rls_set_state_host(self._h, _dp(theta), _dp(P), _dp(lam)), "set_state")

    def state(self):
        """(theta [B,4,4], P [B,4,4,4], lambda [B,4], F [B,4], e [B,4]) after the last tick"""
        th = np.empty((self.B, 4, 4)); P = np.empty((self.B, 4, 4, 4)); lam = np.empty((self.B, 4))
        F = np.empty((self.B, 4)); e = np.empty((self.B, 4))
        self._chk(self._L.brov_rls_get_state_host(self._h, _dp(th), _dp(P), _dp(lam), _dp(F), _dp(e)), "get_state")
        return th, P, lam, F, e

    def update(self, y, acc, vel, rpy, stream=0):
        y = _arr(y, (self.B, 4)); acc = _arr(acc, (self.B, 4)); vel = _arr(vel, (self.B, 4)); rpy = _arr(rpy, (self.B, 3))
        self._chk(self._L.brov_rls_update_host(self._h, _dp(y), _dp(acc), _dp(vel), _dp(rpy), C.c_void_p(stream)), "update")

    def update_device(self, y_ptr, acc_ptr, vel_ptr, rpy_ptr, stream=0):
        self._chk(self._L.brov_rls_update_device(self._h, C.c_void_p(y_ptr), C.c_void_p(acc_ptr), C.c_void_p(vel_ptr),
                                                 C.c_void_p(rpy_ptr), C.c_void_p(stream)), "update_device")

    def update_from_ekf(self, ekf, solver: BatchSolver, stream=0):
        self._chk(self._L.brov_rls_update_from_ekf(self._h, ekf._h, solver._h, C.c_void_p(stream)), "update_from_ekf")

    def apply_to_solver(self, solver: BatchSolver, mode=APPLY_DISTURBANCE, stream=0):
        self._chk(self._L.brov_rls_apply_to_solver(self._h, solver._h, int(mode), C.c_void_p(stream)), "apply_to_solver")

    def outputs(self):
        """(NMPC parameters p[0..3] [B,4], world-frame disturbance wf_env [B,6], status [B])"""
        mp = np.empty((self.B, 4)); wf = np.empty((self.B, 6)); st = np.empty(self.B, dtype=np.int32)
        self._chk(self._L.brov_rls_get_outputs_host(self._h, _dp(mp), _dp(wf), st.ctypes.data_as(C.POINTER(C.c_int32))), "outputs")
        return mp, wf, st

    def theta_device_ptr(self):
        return self._L.brov_rls_theta_device(self._h)

    def last_update_seconds(self):
        s = C.c_double()
        self._chk(self._L.brov_rls_last_update_seconds(self._h, C.byref(s)), "last_update_seconds")
        return s.value
