"""brov_tick_host's transport -- which input set of the pinned staging buffer a tick uses, whether its kernel reads the inputs there or
behind an upload, how the device copies are refreshed and how the records come back -- must not show in any result.  Every case drives one
solver through tick() / tick_inplace() and a second one through setters + solve() + results() and compares bit for bit, on the three
transports: (N, B) = (20, 3) the mailbox with the fused kernel, (20, 65) the bulk path just above the mailbox's 64 instances, (24, 1) the
mailbox with the resident windowed kernel behind the parallel-in-time kernel."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(20, 3), (20, 65), (24, 1)]


@pytest.fixture(scope="module")
def ba():
    import torch
    assert torch.cuda.is_available()
    import bluerov2_amd
    return bluerov2_amd


class _Case:
    """inputs of tick k (x0, window, per-stage parameters: all of them change from tick to tick) and the two solvers"""

    def __init__(self, ba, golden_traj, N, B, seed):
        rng = np.random.default_rng(seed)
        circ = golden_traj["circle"]
        self.N, self.B = N, B
        self.x0 = np.zeros((B, 12)); self.x0[:, :6] = circ[0, :6]
        self.x0 += rng.normal(size=(B, 12)) * np.array([0.05] * 3 + [0.02] * 3 + [0.05] * 3 + [0.02] * 3)
        self.x0[:, :3] += 2.5 * rng.uniform(-1, 1, (B, 3))
        self.win = np.concatenate([circ, np.repeat(circ[-1:], 200, axis=0)])
        self.p = np.ascontiguousarray(np.broadcast_to(ba.P_NOMINAL, (B, N + 1, 16))).copy()
        self.p[:, :, 0] = np.linspace(-5, 5, B)[:, None]
        self.ref = ba.BatchSolver(B, ba.SolverOptions(N, 1.0 / N))
        self.s = ba.BatchSolver(B, ba.SolverOptions(N, 1.0 / N))

    def x(self, k):
        return self.x0 + 0.01 * k

    def y(self, k):
        return np.ascontiguousarray(self.win[k:k + self.N + 1])

    def par(self, k):
        q = self.p.copy(); q[:, :, 1] = 0.5 * k
        return q

    def ref_step(self, x0=None, yref=None, params=None):
        """the reference solver's tick: the setters of the inputs passed, solve(), results()"""
        if x0 is not None: self.ref.set_x0(x0)
        if yref is not None: self.ref.set_yref(yref)
        if params is not None: self.ref.set_params(params)
        self.ref.solve()
        return self.ref.results()

    def same_iterate(self):
        return all(np.array_equal(a, b) for a, b in zip(self.ref.get_iterate(), self.s.get_iterate()))

    def close(self):
        self.ref.close(); self.s.close()


@pytest.mark.parametrize("knob", ["BROV_TICK_ZEROCOPY", "BROV_TICK_BULK"])
@pytest.mark.parametrize("N,B", SHAPES)
def test_knob_fallbacks_give_the_same_ticks(ba, golden_traj, N, B, knob):
    """BROV_TICK_ZEROCOPY=0 (every input uploaded ahead of the kernel) and BROV_TICK_BULK=0 (batches above 64: records copied back behind the
    kernel), each on its own: 6 ticks that rewrite all three inputs on ticks 0 and 3 and pass no x0 on tick 2."""
    c = _Case(ba, golden_traj, N, B, seed=61)
    before = os.environ.get(knob)
    os.environ[knob] = "0"
    try:
        c.s.reload_knobs()
        for k in range(6):
            xk = c.x(k) if k != 2 else None
            pk = c.par(k) if k in (0, 3) else None
            ra = c.ref_step(xk, c.y(k), pk)
            rb = c.s.tick(x0=xk, yref=c.y(k), params=pk)
            assert ra.tobytes() == rb.tobytes(), k
            assert c.s.results().tobytes() == ra.tobytes(), k   # the device-side records are the same ones
        assert c.same_iterate()
    finally:
        os.environ.pop(knob, None)
        if before is not None:
            os.environ[knob] = before
        c.close()


@pytest.mark.parametrize("N,B", SHAPES)
def test_inplace_and_copying_ticks_mixed_on_one_solver(ba, golden_traj, N, B):
    """A caller that holds the staging buffers (tick_buffers: input set 0) and now and then ticks with arrays of its own: those copying ticks
    use the second input set, so after each of them the views still hold, byte for byte, what the caller last wrote there."""
    c = _Case(ba, golden_traj, N, B, seed=62)
    buf = c.s.tick_buffers()
    try:
        for k in range(8):
            if k % 2 == 0:
                buf["x0"][...] = c.x(k); buf["yref"][...] = c.y(k)
                if k == 0:
                    buf["params"][...] = c.par(0)
                mine = {f: buf[f].tobytes() for f in ("x0", "yref", "params")}
                ra = c.ref_step(c.x(k), c.y(k), c.par(0) if k == 0 else None)
                rb = c.s.tick_inplace(x0=True, yref=True, params=k == 0)
            else:
                ra = c.ref_step(c.x(k), c.y(k))
                rb = c.s.tick(x0=c.x(k), yref=c.y(k))
                for f in ("x0", "yref", "params"):
                    assert buf[f].tobytes() == mine[f], (k, f)
            assert ra.tobytes() == rb.tobytes(), k
        assert c.same_iterate()
    finally:
        c.close()


@pytest.mark.parametrize("N,B", SHAPES)
def test_device_copies_are_refreshed_after_a_subset_tick(ba, golden_traj, N, B):
    """Whatever a tick's kernel read in the pinned buffer, the device arrays every other entry point works on hold it afterwards: the getters
    return what was last passed for each input, after ticks that passed all three, x0 only, the window only, the parameters only, all three."""
    c = _Case(ba, golden_traj, N, B, seed=63)
    last = {}
    try:
        for k, subset in enumerate(["xyp", "x", "y", "p", "xyp"]):
            xk = c.x(k) if "x" in subset else None
            yk = c.y(k) if "y" in subset else None
            pk = c.par(k) if "p" in subset else None
            last.update({n: v for n, v in (("x", xk), ("y", yk), ("p", pk)) if v is not None})
            ra = c.ref_step(xk, yk, pk)
            rb = c.s.tick(x0=xk, yref=yk, params=pk)
            assert ra.tobytes() == rb.tobytes(), (k, subset)
            assert np.array_equal(c.s.get_x0(), last["x"]), (k, subset)
            got_y = c.s.get_yref()
            assert all(np.array_equal(got_y[b], last["y"]) for b in range(B)), (k, subset)
            assert np.array_equal(c.s.get_params(), last["p"]), (k, subset)
        assert c.same_iterate()
    finally:
        c.close()


@pytest.mark.parametrize("N,B", [(20, 3), (24, 1)])
def test_split_tick_through_the_channel_leaves_nothing_behind(ba, golden_traj, N, B):
    """tick(yref, params, rti_phase=1) then tick(x0, rti_phase=2) are brov_solve_phase 1 then 2 behind the setters; a plain solve() on the null
    stream that follows is the reference's next step: nothing of the tick's launch inputs outlives the call."""
    c = _Case(ba, golden_traj, N, B, seed=64)
    try:
        for k in range(3):
            c.ref.set_yref(c.y(k)); c.ref.set_params(c.par(k))
            assert c.ref._L.brov_solve_phase(c.ref._h, C.c_void_p(0), 1) == 0
            c.ref.set_x0(c.x(k))
            assert c.ref._L.brov_solve_phase(c.ref._h, C.c_void_p(0), 2) == 0
            ra = c.ref.results()
            c.s.tick(yref=c.y(k), params=c.par(k), rti_phase=1)
            rb = c.s.tick(x0=c.x(k), rti_phase=2)
            assert ra.tobytes() == rb.tobytes(), k
            assert c.ref.last_kernel_path() == c.s.last_kernel_path() == 3
            c.ref.solve(); c.s.solve()
            assert c.ref.results().tobytes() == c.s.results().tobytes(), k
            assert np.array_equal(c.ref.get_x0(), c.s.get_x0()) and np.array_equal(c.ref.get_x0(), c.x(k))
        assert c.same_iterate()
    finally:
        c.close()
