// wrench_source.hpp -- the host side of the world-frame wrench generator (plant_wrench.hip), written once for its two owners: the plant of a
// brov_solver (brov_plant_wrench_*, one wrench per instance) and the vehicles of a brov_fleet (brov_vehicle_wrench_*, one per vehicle).  Each
// public entry point checks its own handle and forwards here with its owner's call context (CallCtx, host_common.hpp), whose wait is for what
// may still read the buffers and is called once the arguments have passed: a refused call waits for nothing.
// Host code only, header only.
#pragma once
#include <cmath>
#include <string>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

struct WrenchSource {
    static constexpr double kWrenchMaxHalfPeriods = 4194304.0;   // 2^22: the half-period index has 22 bits of the amplitude counter
    WrenchGen gen;                 // the generator in force (mode OFF: none, the plant kernels as they always were)
    size_t B = 0;                  // instances the buffers below are sized for, set by the owner at create
    long long tick = 0;            // steps so far (seek sets it): the tick the next step evaluates
    // [B][6] constant mode, [B] table mode, [B][6] eval_host: allocated from the owner's DeviceAllocs, on first use unless reserve() was called
    double *w_const = nullptr, *gain = nullptr, *eval = nullptr;
    double* tab = nullptr;         // [rows][6] table mode, replaced by every upload: not in the owner's DeviceAllocs, freed by destroy()

    int mode() const { return gen.mode; }
    bool off() const { return gen.mode == BROV_WRENCH_OFF; }
    int set_off() { gen.mode = BROV_WRENCH_OFF; return BROV_OK; }
    void destroy() { if (tab) (void)hipFree(tab); tab = nullptr; }

    // the periodic generator's half-period index at tick `t` must fit its counter field
    static int tick_ok(const WrenchGen& g, long long t, const CallCtx& c) {
        if (t < 0) return c.refuse("negative wrench tick");
        if (g.mode == BROV_WRENCH_PERIODIC && !(std::floor((g.phase0 + (double)t * g.dphi) / 3.14159265358979323846) < kWrenchMaxHalfPeriods))
            return c.refuse("the periodic wrench's half-period index floor(t / pi) must stay below 2^22");
        return BROV_OK;
    }
    // are the next `n` steps from the counter in range?  The last of them decides: the phase does not decrease with the tick (dphi >= 0)
    int steps_ok(long long n, const CallCtx& c) const { return n > 0 ? tick_ok(gen, tick + n - 1, c) : BROV_OK; }

    int need(double** p, size_t n, const CallCtx& c) { return *p ? BROV_OK : c.mem.alloc(p, n, c.err); }
    // every buffer now, for an owner that enqueues steps which read `eval` without a host wait (brov_fleet)
    int reserve(const CallCtx& c) {
        if (int rc = need(&w_const, B * 6, c)) return rc;
        if (int rc = need(&gain, B, c)) return rc;
        return need(&eval, B * 6, c);
    }

    // The setters: the context's wait is for every step in flight that may still read the buffers.  A refused call changes nothing.
    int constant_host(const double* w, const CallCtx& c) {
        if (!w) return c.refuse("null argument");
        if (int rc = c.wait()) return rc;
        if (int rc = need(&w_const, B * 6, c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(w_const, w, B * 6 * sizeof(double), hipMemcpyHostToDevice));
        gen.mode = BROV_WRENCH_CONSTANT; gen.w = w_const;
        return BROV_OK;
    }
    int periodic(uint64_t seed, double scale, double phase0, double dphi, double tz_div, const CallCtx& c) {
        if (!std::isfinite(scale) || !(phase0 >= 0.0) || !(dphi >= 0.0) || !std::isfinite(phase0) || !std::isfinite(dphi) || !std::isfinite(tz_div) ||
            tz_div == 0.0)
            return c.refuse("scale, phase0 >= 0, dphi >= 0 and tz_div != 0 must be finite");
        WrenchGen g = gen;   // checked at the counter's tick before it comes into force
        g.mode = BROV_WRENCH_PERIODIC; g.seed = seed; g.scale = scale; g.phase0 = phase0; g.dphi = dphi; g.tz_div = tz_div;
        if (int rc = tick_ok(g, tick, c)) return rc;
        gen = g;
        return BROV_OK;
    }
    int table_host(const double* table, int rows, const double* gain_host, const CallCtx& c) {
        if (!table || rows < 1) return c.refuse("needs a table and rows >= 1");
        if (int rc = c.wait()) return rc;
        if (gain_host) { if (int rc = need(&gain, B, c)) return rc; }
        ScopedDeviceBuffer<double> nt;   // the table in force stays until the new one is complete
        BROV_HIPCHK(c.err, nt.init((size_t)rows * 6));
        BROV_HIPCHK(c.err, hipMemcpy(nt.p, table, (size_t)rows * 6 * sizeof(double), hipMemcpyHostToDevice));
        if (gain_host) BROV_HIPCHK(c.err, hipMemcpy(gain, gain_host, B * sizeof(double), hipMemcpyHostToDevice));
        destroy();
        tab = nt.release();
        gen.mode = BROV_WRENCH_TABLE; gen.tab = tab; gen.rows = rows; gen.gain = gain_host ? gain : nullptr;
        return BROV_OK;
    }
    int seek(int64_t t, const CallCtx& c) {
        if (int rc = tick_ok(gen, (long long)t, c)) return rc;
        tick = (long long)t;
        return BROV_OK;
    }
    // the wrench of every instance at tick `t` to the host (mode OFF: zeros), evaluated on `st` (read once `w` has passed) after the wait; moves nothing
    int eval_host(int64_t t, double* w, const hipStream_t& st, const CallCtx& c) {
        if (!w) return c.refuse("null argument");
        if (int rc = tick_ok(gen, (long long)t, c)) return rc;
        if (int rc = c.wait()) return rc;
        if (int rc = need(&eval, B * 6, c)) return rc;
        launch_wrench_eval(gen, (int)B, (long long)t, eval, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        BROV_HIPCHK(c.err, hipMemcpy(w, eval, B * 6 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
};

}  // namespace brov
