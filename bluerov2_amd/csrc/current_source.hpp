// current_source.hpp -- the host side of the plant's ocean current (plant_current.hip: current_eval_kernel, plant_current_kernel; the public
// names are brov_current_* of include/bluerov2_nmpc.h): the generator in force, its device buffers -- the Gauss-Markov state among them --
// and the timing of the last plant step under a current.  Its owner is a brov_solver or, at batch V, a brov_fleet, whose entry points check their own handle and forward
// here with the owner's call context (CallCtx, host_common.hpp): its wait, for what may still read or write the buffers, is called once the
// arguments have passed, so a refused call changes nothing and waits for nothing.  Host code only, header only.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

struct CurrentSource : PlantStage {   // on: a mode is in force (off: the plant kernels as they always were)
    static constexpr long long kCurrentMaxTicks = 4194304;   // 2^22: the tick has 22 bits of the Gauss-Markov draw's counter
    CurrentGen gen;                // the generator in force
    // [B][3] constant mode, [B] table gain, [B][3] eval_host / get_state_host, [B][3] Gauss-Markov state and mean, [B][3] last applied: from
    // the owner's DeviceAllocs, zeroed, on first use
    double *v_const = nullptr, *gain = nullptr, *eval = nullptr, *state = nullptr, *mean = nullptr, *last = nullptr;
    double* tab = nullptr;         // [rows][3] table mode, replaced by every upload: not in the owner's DeviceAllocs, freed by destroy()

    int mode() const { return gen.mode; }
    bool off() const { return gen.mode == BROV_CURRENT_OFF; }
    int set_off() { gen.mode = BROV_CURRENT_OFF; return PlantStage::set_off(); }
    void destroy() { if (tab) (void)hipFree(tab); tab = nullptr; PlantStage::destroy(); }

    static bool finite(const double* v, size_t n) {
        for (size_t j = 0; v && j < n; j++) if (!std::isfinite(v[j])) return false;
        return true;
    }
    // the Gauss-Markov draws of the next `n` steps from counter tick `t` must fit the counter's tick field
    int steps_ok(long long t, long long n, const CallCtx& c) const {
        if (gen.mode == BROV_CURRENT_GAUSS_MARKOV && n > 0 && t + n > kCurrentMaxTicks)
            return c.refuse("the Gauss-Markov current draws at the plant's tick, which must stay below 2^22");
        return BROV_OK;
    }
    // behind the owner's wait: the buffers every mode and every read-out share
    int ready(const CallCtx& c) {
        if (int rc = c.wait()) return rc;
        if (int rc = buffer(&last, B * 3, c)) return rc;
        gen.last = last;
        return buffer(&eval, B * 3, c);
    }
    void enter(int m) { gen.mode = m; on = true; configured = true; }

    int constant_host(const double* v, const CallCtx& c) {
        if (!v) return c.refuse("null argument");
        if (!finite(v, B * 3)) return c.refuse("the current must be finite");
        if (int rc = ready(c)) return rc;
        if (int rc = buffer(&v_const, B * 3, c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(v_const, v, B * 3 * sizeof(double), hipMemcpyHostToDevice));
        gen.v = v_const;
        enter(BROV_CURRENT_CONSTANT);
        return BROV_OK;
    }
    int table_host(const double* table, int rows, const double* gain_host, const CallCtx& c) {
        if (!table || rows < 1) return c.refuse("needs a table and rows >= 1");
        if (!finite(table, (size_t)rows * 3) || !finite(gain_host, B)) return c.refuse("table and gain must be finite");
        if (int rc = ready(c)) return rc;
        if (gain_host) { if (int rc = buffer(&gain, B, c)) return rc; }
        ScopedDeviceBuffer<double> nt;   // the table in force stays until the new one is complete
        BROV_HIPCHK(c.err, nt.init((size_t)rows * 3));
        BROV_HIPCHK(c.err, hipMemcpy(nt.p, table, (size_t)rows * 3 * sizeof(double), hipMemcpyHostToDevice));
        if (gain_host) BROV_HIPCHK(c.err, hipMemcpy(gain, gain_host, B * sizeof(double), hipMemcpyHostToDevice));
        if (tab) (void)hipFree(tab);
        tab = nt.release();
        gen.tab = tab; gen.rows = rows; gen.gain = gain_host ? gain : nullptr;
        enter(BROV_CURRENT_TABLE);
        return BROV_OK;
    }
    // the state becomes the mean: brov_current_set_state_host chooses another start
    int gauss_markov_host(uint64_t seed, const double* mean_h, const double* mu, const double* amp, const double* lo, const double* hi, double step,
                          const CallCtx& c) {
        if (!mean_h || !mu || !amp) return c.refuse("null argument (needs mean, mu and amp)");
        if (!finite(mean_h, B * 3) || !finite(mu, 3) || !finite(amp, 3) || !finite(lo, 3) || !finite(hi, 3) || !std::isfinite(step))
            return c.refuse("mean, mu, amp, lo, hi and step must be finite");
        if (step < 0.0) return c.refuse("step < 0");
        for (int i = 0; i < 3; i++)
            if ((lo ? lo[i] : -5.0) > (hi ? hi[i] : 5.0)) return c.refuse("lo[i] > hi[i]: a pair of bounds is empty");
        if (int rc = ready(c)) return rc;
        if (int rc = buffer(&state, B * 3, c)) return rc;
        if (int rc = buffer(&mean, B * 3, c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(mean, mean_h, B * 3 * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(c.err, hipMemcpy(state, mean_h, B * 3 * sizeof(double), hipMemcpyHostToDevice));
        gen.c = state; gen.mean = mean; gen.seed = seed; gen.step = step;
        for (int i = 0; i < 3; i++) { gen.mu[i] = mu[i]; gen.amp[i] = amp[i]; gen.lo[i] = lo ? lo[i] : -5.0; gen.hi[i] = hi ? hi[i] : 5.0; }
        enter(BROV_CURRENT_GAUSS_MARKOV);
        return BROV_OK;
    }
    // the generator at tick `t` into `eval` on `st` and to the host; the caller has checked the mode and called ready()
    int evaluate(long long t, double* v, const hipStream_t& st, const CallCtx& c) {
        launch_current_eval(gen, (int)B, t, eval, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        BROV_HIPCHK(c.err, hipMemcpy(v, eval, B * 3 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    // constant / table (OFF: zeros) at tick `t`; moves nothing
    int eval_host(int64_t t, double* v, const hipStream_t& st, const CallCtx& c) {
        if (!v) return c.refuse("null argument");
        if (t < 0) return c.refuse("negative tick");
        if (gen.mode == BROV_CURRENT_GAUSS_MARKOV)
            return c.refuse("the Gauss-Markov current is a state, not a function of the tick (brov_current_get_state_host)");
        if (int rc = ready(c)) return rc;
        return evaluate((long long)t, v, st, c);
    }
    // what the next plant step, at counter tick `t`, applies: the Gauss-Markov state, else the generator at that tick
    int get_state_host(long long t, double* v, const hipStream_t& st, const CallCtx& c) {
        if (!v) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        return evaluate(t, v, st, c);
    }
    int set_state_host(const double* v, const CallCtx& c) {
        if (!v) return c.refuse("null argument");
        if (gen.mode != BROV_CURRENT_GAUSS_MARKOV) return c.refuse("only the Gauss-Markov current has a state (brov_current_gauss_markov_host)");
        if (!finite(v, B * 3)) return c.refuse("the state must be finite");
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(state, v, B * 3 * sizeof(double), hipMemcpyHostToDevice));
        return BROV_OK;
    }
    int last_host(double* v, const CallCtx& c) {
        if (!v) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(v, last, B * 3 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int last_seconds(double* seconds, const CallCtx& c) { return PlantStage::last_seconds(seconds, "no plant step under a current yet", c); }
    // an owner's reset (brov_fleet_reset), behind its wait: the Gauss-Markov state back to its mean, `last` to zeros; mode and settings stay
    int rewind(std::string& err) {
        if (state && mean) BROV_HIPCHK(err, hipMemcpy(state, mean, B * 3 * sizeof(double), hipMemcpyDeviceToDevice));
        if (last) BROV_HIPCHK(err, hipMemset(last, 0, B * 3 * sizeof(double)));
        return BROV_OK;
    }

    // one plant step under the current on `st` (the owner has checked the mode), timed; behind the thruster stage where th_on, g.mode OFF: no
    // world wrench on top
    void step(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, double dt, int substeps, double* xlog,
              double* ulog, bool th_on, const ThrusterPar& T, const ThrusterDev& D, const WrenchGen& g, long long tick, double* wlog, hipStream_t st) {
        (void)timer.start(st);
        launch_plant_current(x0, res, pplant, prp, rp_stride, (int)B, dt, substeps, xlog, ulog, th_on, T, D, g, gen, tick, wlog, st);
        (void)timer.stop(st);
    }
};

}  // namespace brov
