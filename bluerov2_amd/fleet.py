"""Host-side mirror of the fleet planning loop (include/bluerov2_nmpc.h, brov_fleet_*): V vehicles x C candidates laid over one
BatchSolver of batch V * C, instance v * C + c = candidate c of vehicle v.  ctypes over the HIP library -- no CPU path."""
import ctypes as C

import numpy as np

from .solver import RESULT_DTYPE, _Handle, _arr, _bind, _dp, _load


def _protos(L):
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.brov_fleet_create.argtypes = [C.POINTER(vp), vp, C.c_int]
    _bind(L, {"brov_fleet_last_error": []}, C.c_char_p)
    _bind(L, {"brov_fleet_destroy": [vp]}, None)
    _bind(L, {
        "brov_fleet_vehicles": [vp], "brov_fleet_candidates": [vp], "brov_fleet_reset": [vp],
        "brov_fleet_set_state_host": [vp, dp], "brov_fleet_get_state_host": [vp, dp], "brov_fleet_set_plant_params_host": [vp, dp],
        "brov_fleet_select_device": [vp, vp, vp, vp, vp], "brov_fleet_select_host": [vp, vp, ip, vp],
        "brov_fleet_step": [vp, vp, C.c_double, C.c_int, vp], "brov_fleet_get_last_host": [vp, dp, ip, ip],
        "brov_closed_loop_fleet": [vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, ip, ip],
        "brov_fleet_last_seconds": [vp, dp],
    })


def _fleet_lib():
    return _load(_protos)


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


class Fleet(_Handle):
    """A fleet over `solver` (brov_fleet): groups of `candidates` consecutive instances are the candidates of one vehicle.  The solver
    must outlive the fleet.  select() = the per-vehicle arg-min alone, step() = select + plant + state broadcast behind a solve,
    closed_loop() = whole planning ticks with one host wait."""
    _last_error, _destroy = "brov_fleet_last_error", "brov_fleet_destroy"

    def __init__(self, solver, candidates):
        L = _fleet_lib()
        self.solver = solver
        self._create(L, "brov_fleet_create", solver._h, int(candidates))
        self.C = int(candidates)
        self.V = solver.B // self.C

    def reset(self):
        """held inputs to zero, every vehicle's state := x0 of its candidate 0, tick counter to zero"""
        self._chk(self._L.brov_fleet_reset(self._h), "reset")

    def set_state(self, xv):
        """vehicle states [V, 12]; also written into x0 of every candidate"""
        self._chk(self._L.brov_fleet_set_state_host(self._h, _dp(_arr(xv, (self.V, 12)))), "set_state")

    def state(self):
        xv = np.empty((self.V, 12))
        self._chk(self._L.brov_fleet_get_state_host(self._h, _dp(xv)), "state")
        return xv

    def set_plant_params(self, p):
        """true parameters of the vehicles [V, 16]; None: stage 0 of candidate 0 of each group, read at every step"""
        self._chk(self._L.brov_fleet_set_plant_params_host(self._h, None if p is None else _dp(_arr(p, (self.V, 16)))), "set_plant_params")

    def select(self, records=None, with_records=True):
        """(winner [V] int32, winning records [V] of RESULT_DTYPE or None) from host records [V * C] (None: the solver's own)"""
        rp = None
        if records is not None:
            records = _arr(records, (self.V * self.C,), RESULT_DTYPE)
            rp = records.ctypes.data_as(C.c_void_p)
        win = np.empty(self.V, dtype=np.int32)
        rec = np.empty(self.V, dtype=RESULT_DTYPE) if with_records else None
        self._chk(self._L.brov_fleet_select_host(self._h, rp, _ip(win), None if rec is None else rec.ctypes.data_as(C.c_void_p)), "select")
        return win, rec

    def select_device(self, rec_ptr, winner_ptr, winner_rec_ptr=None, stream=0):
        """the same through device pointers (rec_ptr 0 / None: the solver's records); enqueued on `stream`, no host wait"""
        self._chk(self._L.brov_fleet_select_device(self._h, C.c_void_p(rec_ptr or None), C.c_void_p(winner_ptr), C.c_void_p(winner_rec_ptr or None),
                                                   C.c_void_p(stream)), "select_device")

    def step(self, rec_ptr=None, dt=0.05, substeps=1, stream=0):
        """select + plant + broadcast from device records (None: the solver's); enqueued on `stream`"""
        self._chk(self._L.brov_fleet_step(self._h, C.c_void_p(rec_ptr or None), float(dt), int(substeps), C.c_void_p(stream)), "step")

    def last(self):
        """(u [V, 4], status [V], winner [V]) of the last step"""
        u = np.empty((self.V, 4)); st = np.empty(self.V, dtype=np.int32); win = np.empty(self.V, dtype=np.int32)
        self._chk(self._L.brov_fleet_get_last_host(self._h, _dp(u), _ip(st), _ip(win)), "last")
        return u, st, win

    def closed_loop(self, ticks, t0=0.0, dt_ref=0.05, dt_node=0.05, dt=0.05, substeps=1, log=True):
        """`ticks` planning ticks (candidate windows at t0 + k * dt_ref -> solve -> step), one host wait.  With log: (u [ticks, V, 4],
        x [ticks + 1, V, 12], status [ticks, V], winner [ticks, V])"""
        ticks = int(ticks)
        u = x = st = win = None
        if log:
            n = max(ticks, 0)
            u = np.empty((n, self.V, 4)); x = np.empty((n + 1, self.V, 12))
            st = np.empty((n, self.V), dtype=np.int32); win = np.empty((n, self.V), dtype=np.int32)
        self._chk(self._L.brov_closed_loop_fleet(self._h, ticks, float(t0), float(dt_ref), float(dt_node), float(dt), int(substeps), _dp(u), _dp(x),
                                                 _ip(st), _ip(win)), "closed_loop")
        return (u, x, st, win) if log else None

    def last_seconds(self):
        """seconds of the last select kernel"""
        s = C.c_double()
        self._chk(self._L.brov_fleet_last_seconds(self._h, C.byref(s)), "last_seconds")
        return s.value
