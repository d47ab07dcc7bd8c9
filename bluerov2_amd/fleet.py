"""Host-side mirror of the fleet planning loop (include/bluerov2_nmpc.h, brov_fleet_*, brov_vehicle_*): V vehicles x C candidates laid over
one BatchSolver of batch V * C, instance v * C + c = candidate c of vehicle v; a world-frame wrench per vehicle and a BatchEkf of batch V
closing the loop.  ctypes over the HIP library -- no CPU path."""
import ctypes as C

import numpy as np

from .solver import RESULT_DTYPE, _Handle, _Wrench, _arr, _arr_opt, _bind, _dp, _load


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
        "brov_vehicle_wrench_constant_host": [vp, dp], "brov_vehicle_wrench_periodic": [vp, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double],
        "brov_vehicle_wrench_table_host": [vp, dp, C.c_int, dp], "brov_vehicle_wrench_off": [vp], "brov_vehicle_wrench_mode": [vp],
        "brov_vehicle_wrench_seek": [vp, C.c_int64], "brov_vehicle_wrench_eval_host": [vp, C.c_int64, dp],
        "brov_vehicle_observe": [vp, vp, C.c_double, vp], "brov_vehicle_apply_estimate": [vp, vp, vp],
        "brov_closed_loop_fleet_dob": [vp, vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, dp, dp, ip, ip, dp, dp],
    })
    _bind(L, {"brov_vehicle_wrench_tick": [vp]}, C.c_int64)
    _bind(L, {
        "brov_vehicle_current_constant_host": [vp, dp], "brov_vehicle_current_table_host": [vp, dp, C.c_int, dp],
        "brov_vehicle_current_gauss_markov_host": [vp, C.c_uint64, dp, dp, dp, dp, dp, C.c_double], "brov_vehicle_current_off": [vp],
        "brov_vehicle_current_mode": [vp], "brov_vehicle_current_eval_host": [vp, C.c_int64, dp], "brov_vehicle_current_get_state_host": [vp, dp],
        "brov_vehicle_current_set_state_host": [vp, dp], "brov_vehicle_current_last_host": [vp, dp],
        "brov_vehicle_coriolis_set": [vp, C.c_int, C.c_double, C.c_double], "brov_vehicle_coriolis_off": [vp], "brov_vehicle_coriolis_terms": [vp],
        "brov_vehicle_coriolis_get": [vp, C.POINTER(C.c_int), dp, dp], "brov_vehicle_coriolis_eval_host": [vp, dp, dp, dp],
        "brov_vehicle_coriolis_last_host": [vp, dp],
    })
    _bind(L, {
        "brov_clearance_set": [vp, C.c_double, C.c_double, C.c_int], "brov_clearance_off": [vp], "brov_clearance_enabled": [vp],
        "brov_clearance_set_plan_host": [vp, dp], "brov_clearance_get_plan_host": [vp, dp],
        "brov_clearance_eval_device": [vp, vp, vp, vp, vp, vp], "brov_clearance_eval_host": [vp, vp, dp, vp],
        "brov_clearance_get_stats_host": [vp, dp, dp, ip], "brov_clearance_last_seconds": [vp, dp],
        "brov_clearance_dev_set_slices": [vp, C.c_int], "brov_clearance_dev_slices": [vp],
    })
    _bind(L, STANDOFF_PROTOS)


# the stand-off term, include/bluerov2_nmpc_standoff.h: name -> argument types (every call returns int)
_VP, _DP = C.c_void_p, C.POINTER(C.c_double)
STANDOFF_PROTOS = {
    "brov_standoff_set": [_VP, C.c_double, C.c_double, C.c_double, C.c_int], "brov_standoff_off": [_VP], "brov_standoff_enabled": [_VP],
    "brov_standoff_eval_device": [_VP, _VP, _VP, _VP, _VP, _VP, _VP], "brov_standoff_eval_host": [_VP, _VP, _DP, _VP, C.POINTER(C.c_int64)],
    "brov_standoff_get_stats_host": [_VP, _DP, _DP, C.POINTER(C.c_int32)], "brov_standoff_last_seconds": [_VP, _DP],
}


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
        """held inputs to zero, every vehicle's state := x0 of its candidate 0, tick counter to zero, a Gauss-Markov current to its mean"""
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

    # ---- the fleet under disturbance (brov_vehicle_*) -------------------------------------------------------------------------------
    _wrench = property(lambda self: _Wrench(self, "brov_vehicle_wrench_", self.V, "set_wrench"))

    def set_wrench(self, constant=None, periodic=None, table=None, gain=None):
        """the vehicles' world-frame wrench, BatchSolver.set_plant_wrench at batch V: exactly one of
            constant=w         [6] or [V, 6], world frame [fx fy fz tx ty tz]
            periodic=dict(seed=0, scale=6.0, phase0=0.0, dphi=0.125, tz_div=3.0)   (any subset)
            table=tab          [rows, 6], row min(tick, rows - 1); gain=[V] scales it per vehicle"""
        self._wrench.set(constant, periodic, table, gain)

    def wrench_off(self):
        self._wrench.call("off")

    def wrench_mode(self):
        return self._wrench.get("mode")

    def wrench(self, tick):
        """[V, 6]: the wrench of every vehicle at `tick`, evaluated by the device generator (moves nothing; zeros while off)"""
        return self._wrench.eval(tick)

    def wrench_seek(self, tick):
        self._wrench.call("seek", int(tick))

    def wrench_tick(self):
        """the tick counter: fleet steps since the last reset or seek (step and every closed-loop tick add one)"""
        return self._wrench.get("tick")

    # ---- the water the vehicles move in (brov_vehicle_current_*, brov_vehicle_coriolis_*) ---------------------------------------------------
    def _rows(self, v, shape, name):
        """v broadcast to `shape` as a contiguous float64 array (None stays None); a shape that does not broadcast is a ValueError"""
        if v is None:
            return None
        try:
            return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), shape))
        except ValueError:
            raise ValueError(f"{name} must be {list(shape)} (or broadcast to it), got {list(np.shape(v))}") from None

    def set_current(self, constant=None, table=None, gain=None, gauss_markov=None):
        """the fleet steps from now on run in moving water, BatchSolver.set_current at batch V with the vehicle as instance: exactly one of
            constant=      [3] for all or [V, 3], world-frame (vx, vy, vz) in m/s
            table=         [rows, 3], one row per fleet step (wrench_tick()), the last row repeated; gain= [V] scales it per vehicle: one
                           body of water and V vehicles in it
            gauss_markov=  dict(mean [3] or [V, 3], mu, amp: scalar or [3]; optional seed=0, lo=-5, hi=5: scalar or [3], step=0.05)"""
        if (constant is not None) + (table is not None) + (gauss_markov is not None) != 1:
            raise ValueError("set_current takes exactly one of constant=, table=, gauss_markov=")
        if gain is not None and table is None:
            raise ValueError("gain= goes with table=")
        if constant is not None:
            self._chk(self._L.brov_vehicle_current_constant_host(self._h, _dp(self._rows(constant, (self.V, 3), "constant"))), "set_current")
        elif table is not None:
            tab = np.ascontiguousarray(table, dtype=np.float64)
            if tab.ndim != 2 or tab.shape[1] != 3 or tab.shape[0] < 1:
                raise ValueError("current table must be [rows][3]")
            self._chk(self._L.brov_vehicle_current_table_host(self._h, _dp(tab), tab.shape[0], _dp(_arr_opt(gain, (self.V,)))), "set_current")
        else:
            kw = dict(seed=0, mean=None, mu=None, amp=None, lo=None, hi=None, step=0.05)
            unknown = set(gauss_markov) - set(kw)
            if unknown:
                raise ValueError(f"unknown Gauss-Markov current parameters {sorted(unknown)}")
            kw.update(gauss_markov)
            if kw["mean"] is None or kw["mu"] is None or kw["amp"] is None:
                raise ValueError("gauss_markov= needs mean, mu and amp")
            r = self._rows
            self._chk(self._L.brov_vehicle_current_gauss_markov_host(
                self._h, int(kw["seed"]) & 0xFFFFFFFFFFFFFFFF, _dp(r(kw["mean"], (self.V, 3), "mean")), _dp(r(kw["mu"], (3,), "mu")),
                _dp(r(kw["amp"], (3,), "amp")), _dp(r(kw["lo"], (3,), "lo")), _dp(r(kw["hi"], (3,), "hi")), float(kw["step"])), "set_current")

    def current_off(self):
        """still water; with the Coriolis stage off too, the plant kernels as they always were"""
        self._chk(self._L.brov_vehicle_current_off(self._h), "current_off")

    def current_mode(self):
        return int(self._L.brov_vehicle_current_mode(self._h))

    def _current_out(self, fn, name, *args):
        v = np.empty((self.V, 3))
        self._chk(fn(self._h, *args, _dp(v)), name)
        return v

    def current(self, tick):
        """[V, 3]: the constant / table current of every vehicle at `tick`, evaluated by the device generator (moves nothing)"""
        return self._current_out(self._L.brov_vehicle_current_eval_host, "current", int(tick))

    def current_state(self):
        """[V, 3]: the current the next fleet step applies (Gauss-Markov mode: the state)"""
        return self._current_out(self._L.brov_vehicle_current_get_state_host, "current_state")

    def set_current_state(self, v):
        """Gauss-Markov mode: the state, [3] for all or [V, 3]"""
        self._chk(self._L.brov_vehicle_current_set_state_host(self._h, _dp(self._rows(v, (self.V, 3), "the current state"))), "set_current_state")

    def current_last(self):
        """[V, 3]: the current the last fleet step applied (zeros before the first and after reset())"""
        return self._current_out(self._L.brov_vehicle_current_last_host, "current_last")

    def set_coriolis(self, terms, ka=0.0, ma=1.2481):
        """the fleet's plant from now on adds the Coriolis and centripetal forces of `terms` (CORIOLIS_RIGID, CORIOLIS_ADDED or both) at every
        RK stage, with the vehicles' true added masses (set_plant_params) and the roll / pitch added inertia ka, ma"""
        self._chk(self._L.brov_vehicle_coriolis_set(self._h, int(terms), float(ka), float(ma)), "set_coriolis")

    def coriolis_off(self):
        self._chk(self._L.brov_vehicle_coriolis_off(self._h), "coriolis_off")

    def coriolis_terms(self):
        """the CORIOLIS_* bit mask in force, 0 while off"""
        return int(self._L.brov_vehicle_coriolis_terms(self._h))

    def coriolis_eval(self, x, vc=None):
        """[V, 4]: the stage's force [X Y Z N] at the states x [V, 12] in water moving with vc ([3] for all or [V, 3]; None: still water),
        with the parameters the next fleet step would read (moves nothing)"""
        x = _arr(x, (self.V, 12))
        c = np.empty((self.V, 4))
        self._chk(self._L.brov_vehicle_coriolis_eval_host(self._h, _dp(x), _dp(self._rows(vc, (self.V, 3), "vc")), _dp(c)), "coriolis_eval")
        return c

    def coriolis_last(self):
        """[V, 4]: the stage's force at the start state of the last fleet step under it (zeros before the first and after reset())"""
        c = np.empty((self.V, 4))
        self._chk(self._L.brov_vehicle_coriolis_last_host(self._h, _dp(c)), "coriolis_last")
        return c

    def observe(self, ekf, dt=0.05, stream=0):
        """one tick of the observer `ekf` (BatchEkf of batch V) on the vehicles' states, the inputs they were given and (v - v_prev) / dt"""
        self._chk(self._L.brov_vehicle_observe(self._h, ekf._h, float(dt), C.c_void_p(stream)), "observe")

    def apply_estimate(self, ekf, stream=0):
        """p[0..3] of every stage of every candidate of vehicle v := the estimate of vehicle v; needs set_plant_params"""
        self._chk(self._L.brov_vehicle_apply_estimate(self._h, ekf._h, C.c_void_p(stream)), "apply_estimate")

    def closed_loop_dob(self, ekf, ticks, t0=0.0, dt_ref=0.05, dt_node=0.05, dt=0.05, substeps=1, log=True):
        """closed_loop() under the fleet's wrench with observe + apply_estimate behind every step (ekf=None: neither), one host wait.  With
        log: dict(u [ticks, V, 4], x [ticks + 1, V, 12], status [ticks, V], winner [ticks, V], wrench [ticks, V, 6], est [ticks, V, 6] or
        None without an observer)"""
        ticks = int(ticks)
        u = x = st = win = w = est = None
        if log:
            n = max(ticks, 0)
            u = np.empty((n, self.V, 4)); x = np.empty((n + 1, self.V, 12))
            st = np.empty((n, self.V), dtype=np.int32); win = np.empty((n, self.V), dtype=np.int32)
            w = np.empty((n, self.V, 6)); est = np.empty((n, self.V, 6)) if ekf is not None else None
        self._chk(self._L.brov_closed_loop_fleet_dob(self._h, None if ekf is None else ekf._h, ticks, float(t0), float(dt_ref), float(dt_node),
                                                     float(dt), int(substeps), _dp(u), _dp(x), _ip(st), _ip(win), _dp(w), _dp(est)), "closed_loop_dob")
        return dict(u=u, x=x, status=st, winner=win, wrench=w, est=est) if log else None

    # ---- the inter-vehicle clearance term (brov_clearance_*) ------------------------------------------------------------------------
    def set_clearance(self, radius, weight=float("inf"), shift=1):
        """turns the term on: candidates that come closer than `radius` to another vehicle's plan pay weight * (radius^2 - d2min) on their
        cost ahead of the select (weight=inf: they are ineligible); the plan of a peer is read `shift` stages ahead.  step() and the closed
        loops then re-score, select and publish the winners' paths as the new plans"""
        self._chk(self._L.brov_clearance_set(self._h, float(radius), float(weight), int(shift)), "set_clearance")

    def clearance_off(self):
        """today's step again; plan, statistics and parameters are kept"""
        self._chk(self._L.brov_clearance_off(self._h), "clearance_off")

    def clearance_enabled(self):
        return bool(self._L.brov_clearance_enabled(self._h))

    def set_plan(self, plan):
        """the positions of the path every vehicle committed to, [V, N + 1, 3]"""
        self._chk(self._L.brov_clearance_set_plan_host(self._h, _dp(_arr(plan, (self.V, self.solver.N + 1, 3)))), "set_plan")

    def plan(self):
        plan = np.empty((self.V, self.solver.N + 1, 3))
        self._chk(self._L.brov_clearance_get_plan_host(self._h, _dp(plan)), "plan")
        return plan

    def clearance_eval(self, records=None):
        """(d2min [V * C], re-scored records [V * C]) of the solver's iterate against the plan as it stands, from host records (None: the
        solver's own); moves nothing"""
        B = self.V * self.C
        rp = None
        if records is not None:
            records = _arr(records, (B,), RESULT_DTYPE)
            rp = records.ctypes.data_as(C.c_void_p)
        d2 = np.empty(B)
        out = np.empty(B, dtype=RESULT_DTYPE)
        self._chk(self._L.brov_clearance_eval_host(self._h, rp, _dp(d2), out.ctypes.data_as(C.c_void_p)), "clearance_eval")
        return d2, out

    def clearance_stats(self):
        """dict(last_d2 [V]: d2min of the last step's winner or -1, min_d2 [V]: its minimum over the steps with a winner, below [V]: steps
        whose winner was inside the radius)"""
        last, low, below = np.empty(self.V), np.empty(self.V), np.empty(self.V, dtype=np.int32)
        self._chk(self._L.brov_clearance_get_stats_host(self._h, _dp(last), _dp(low), _ip(below)), "clearance_stats")
        return dict(last_d2=last, min_d2=low, below=below)

    def clearance_slices(self, slices=None):
        """development and tests: the number of grid-level slices the distance kernel cuts the peer range into (set with 1..8, 0: the
        default); the results do not depend on it"""
        if slices is not None:
            self._chk(self._L.brov_clearance_dev_set_slices(self._h, int(slices)), "clearance_slices")
        return int(self._L.brov_clearance_dev_slices(self._h))

    def clearance_seconds(self):
        """seconds of the last distance kernel"""
        s = C.c_double()
        self._chk(self._L.brov_clearance_last_seconds(self._h, C.byref(s)), "clearance_seconds")
        return s.value

    # ---- the stand-off term (brov_standoff_*) ---------------------------------------------------------------------------------------
    def set_standoff(self, radius, weight=float("inf"), reach=None, first=1):
        """turns the term on: candidates whose predicted path (stages first ... N) comes closer than `radius` to the solver's scene -- the boxes
        of set_range_scene and the mesh of set_range_mesh, as they stand at every step -- pay weight * (radius^2 - s2) on their cost ahead of
        the select (weight=inf: they are ineligible).  Distances are capped at `reach` >= radius (None: radius; inf allowed): a small reach
        is what makes the walk over the mesh cheap"""
        self._chk(self._L.brov_standoff_set(self._h, float(radius), float(weight), float(radius if reach is None else reach), int(first)),
                  "set_standoff")

    def standoff_off(self):
        """today's step again; statistics and parameters are kept"""
        self._chk(self._L.brov_standoff_off(self._h), "standoff_off")

    def standoff_enabled(self):
        return bool(self._L.brov_standoff_enabled(self._h))

    def standoff_eval(self, records=None, visits=False):
        """(s2 [V * C], re-scored records [V * C]) of the solver's iterate against the scene as it stands, from host records (None: the
        solver's own); with visits a third item, [V * C, 2] int64: the node tests and triangle tests each candidate's walks made.  Moves
        nothing"""
        B = self.V * self.C
        rp = None
        if records is not None:
            records = _arr(records, (B,), RESULT_DTYPE)
            rp = records.ctypes.data_as(C.c_void_p)
        s2 = np.empty(B)
        out = np.empty(B, dtype=RESULT_DTYPE)
        vis = np.zeros((B, 2), dtype=np.int64) if visits else None
        self._chk(self._L.brov_standoff_eval_host(self._h, rp, _dp(s2), out.ctypes.data_as(C.c_void_p),
                                                  None if vis is None else vis.ctypes.data_as(C.POINTER(C.c_int64))), "standoff_eval")
        return (s2, out, vis) if visits else (s2, out)

    def standoff_stats(self):
        """dict(last_s2 [V]: s2 of the last step's winner or -1, min_s2 [V]: its minimum over the steps with a winner, below [V]: steps
        whose winner was inside the radius)"""
        last, low, below = np.empty(self.V), np.empty(self.V), np.empty(self.V, dtype=np.int32)
        self._chk(self._L.brov_standoff_get_stats_host(self._h, _dp(last), _dp(low), _ip(below)), "standoff_stats")
        return dict(last_s2=last, min_s2=low, below=below)

    def standoff_seconds(self):
        """seconds of the last distance kernel"""
        s = C.c_double()
        self._chk(self._L.brov_standoff_last_seconds(self._h, C.byref(s)), "standoff_seconds")
        return s.value

    def last_seconds(self):
        """seconds of the last select kernel"""
        s = C.c_double()
        self._chk(self._L.brov_fleet_last_seconds(self._h, C.byref(s)), "last_seconds")
        return s.value
