// rotor_source.hpp -- the host side of the plant's rotor stage (rotor_kernel.hip: rotor_shift_kernel, rotor_eval_kernel; the public names are
// brov_rotor_* of include/bluerov2_nmpc.h): the configuration in force -- step, limits and the coefficients, which are computed HERE, in libm
// doubles, and uploaded --, the rotor state, the applied records and the statistics on the device, the stage's own step count and the timing
// of the last shift.  Its owner is a brov_solver, whose entry points check their own handle and forward here with the owner's call context
// (CallCtx, host_common.hpp): its wait, for what may still read or write the buffers, is called once the arguments have passed, so a refused
// call changes nothing and waits for nothing.  Shares PlantStage with the thruster, the sensor and the delay stage.  Host code only, header only.
#pragma once
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

struct RotorSource : PlantStage {   // on: the plant steps read the applied records (off: what they read without the stage)
    RotorPar par;                  // lo, hi in force
    double *alpha = nullptr, *beta = nullptr;   // [B][6] coefficients of the step h, as the host computed them
    double* state = nullptr;       // [B][6] r: the thrust every rotor gives at the end of the last step
    double* last = nullptr;        // [B][6] m: the mean thrusts the last step applied
    double* lag_sq = nullptr;      // [B] running sum of |c - m|^2
    brov_result* applied = nullptr;   // [B] what the last plant step was given
    double* eval = nullptr;        // [4][B][6] of eval_host: commands, state, applied, new state
    std::vector<double> alpha_h, beta_h;   // the host's copy of the coefficients (get_coeffs_host)
    double h = 0.0;                // the step the coefficients were computed for: a plant step of another dt is refused (0: never set)
    bool observer_applied = false; // brov_ekf_update_from_solver reads the applied records
    long long steps = 0;           // steps of the stage since it was set or reset

    // alpha = exp(-h / tau), beta = (1 - alpha) / (h / tau) of the exact solution of r' = (c - r) / tau over h; tau = 0: (0, 0).  Needs no device
    static int coeffs(double tau, double h_, double* al, double* be) {
        if (!al || !be || !(tau >= 0.0) || !std::isfinite(tau) || !std::isfinite(h_) || !(h_ > 0.0)) return BROV_ERR_ARG;
        if (tau == 0.0) { *al = 0.0; *be = 0.0; return BROV_OK; }
        const double x = h_ / tau;
        *al = std::exp(-x);
        *be = -std::expm1(-x) / x;
        return BROV_OK;
    }

    // the buffers on first use; zeroed buffers are the default configuration: every pair (0, 0), the stage a copy, no limits
    int ensure(const CallCtx& c) {
        if (int rc = buffer(&alpha, B * 6, c)) return rc;
        if (int rc = buffer(&beta, B * 6, c)) return rc;
        if (int rc = buffer(&state, B * 6, c)) return rc;
        if (int rc = buffer(&last, B * 6, c)) return rc;
        if (int rc = buffer(&lag_sq, B, c)) return rc;
        if (int rc = buffer(&applied, B, c)) return rc;
        if (int rc = buffer(&eval, 4 * B * 6, c)) return rc;
        if (!configured) {
            const double inf = std::numeric_limits<double>::infinity();
            for (int i = 0; i < 6; i++) { par.lo[i] = -inf; par.hi[i] = inf; }
            alpha_h.assign(B * 6, 0.0); beta_h.assign(B * 6, 0.0);
            configured = true;
        }
        return BROV_OK;
    }
    int ready(const CallCtx& c) { const int rc = c.wait(); return rc ? rc : ensure(c); }
    // state, applied records, statistics and the step count to zero; the caller has waited
    int clear(std::string& err) {
        BROV_HIPCHK(err, hipMemset(state, 0, B * 6 * sizeof(double)));
        BROV_HIPCHK(err, hipMemset(last, 0, B * 6 * sizeof(double)));
        BROV_HIPCHK(err, hipMemset(lag_sq, 0, B * sizeof(double)));
        BROV_HIPCHK(err, hipMemset(applied, 0, B * sizeof(brov_result)));
        steps = 0;
        return BROV_OK;
    }
    int reset(const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        return clear(c.err);
    }

    int set_host(const double* tau, double h_, double Ts, const double* lo, const double* hi, int32_t observer_applied_, const CallCtx& c) {
        if (!std::isfinite(h_)) return c.refuse("h must be finite (<= 0: the options' Ts)");
        const double hh = h_ > 0.0 ? h_ : Ts;
        for (int i = 0; i < 6; i++) {
            const double l = lo ? lo[i] : -1.0, u = hi ? hi[i] : 1.0;
            if (std::isnan(l) || std::isnan(u)) return c.refuse("a command limit is NaN");
            if (lo && hi && l > u) return c.refuse("cmd_lo[i] > cmd_hi[i]: a command limit pair is empty");
        }
        std::vector<double> al(B * 6), be(B * 6);
        for (size_t j = 0; j < B * 6; j++)
            if (coeffs(tau ? tau[j] : 0.2, hh, &al[j], &be[j]) != BROV_OK) return c.refuse("tau must be finite and >= 0, the step positive");
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(alpha, al.data(), B * 6 * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(c.err, hipMemcpy(beta, be.data(), B * 6 * sizeof(double), hipMemcpyHostToDevice));
        alpha_h.swap(al); beta_h.swap(be);
        const double inf = std::numeric_limits<double>::infinity();
        for (int i = 0; i < 6; i++) { par.lo[i] = lo ? lo[i] : -inf; par.hi[i] = hi ? hi[i] : inf; }
        h = hh; observer_applied = observer_applied_ != 0;
        if (int rc = clear(c.err)) return rc;
        on = true;
        return BROV_OK;
    }
    // while the stage is on its coefficients hold for one step length alone
    int dt_ok(double dt, const CallCtx& c) const {
        return on && dt != h ? c.refuse("the rotor stage is on and dt is not the step its coefficients were computed for (brov_rotor_set_host)") : BROV_OK;
    }

    // one step of the stage on `st` ahead of the plant kernel (the owner has checked `on`), timed: `rec` in, `applied` out
    void shift(const brov_result* rec, double* ulog, hipStream_t st) {
        (void)timer.start(st);
        launch_rotor_shift(rec, applied, par, alpha, beta, state, last, lag_sq, (int)B, ulog, st);
        (void)timer.stop(st);
        steps++;
    }

    int set_state_host(const double* r, const CallCtx& c) {
        if (!r) return c.refuse("null argument");
        for (size_t j = 0; j < B * 6; j++)
            if (!std::isfinite(r[j])) return c.refuse("the rotor state must be finite");
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(state, r, B * 6 * sizeof(double), hipMemcpyHostToDevice));
        return BROV_OK;
    }
    int get_state_host(double* r, const CallCtx& c) {
        if (!r) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(r, state, B * 6 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int last_host(double* u0_applied, double* thrust_applied, const CallCtx& c) {
        if (!u0_applied && !thrust_applied) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        if (u0_applied)
            BROV_HIPCHK(c.err, hipMemcpy2D(u0_applied, 4 * sizeof(double), (const char*)applied + offsetof(brov_result, u0), sizeof(brov_result),
                                           4 * sizeof(double), B, hipMemcpyDeviceToHost));
        if (thrust_applied) BROV_HIPCHK(c.err, hipMemcpy(thrust_applied, last, B * 6 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_stats_host(double* lag_sq_out, int64_t* steps_out, const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        if (lag_sq_out) BROV_HIPCHK(c.err, hipMemcpy(lag_sq_out, lag_sq, B * sizeof(double), hipMemcpyDeviceToHost));
        if (steps_out) *steps_out = (int64_t)steps;
        return BROV_OK;
    }
    int get_coeffs_host(double* al, double* be, double* h_out, const CallCtx& c) {
        if (!al && !be && !h_out) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        for (size_t j = 0; j < B * 6; j++) {
            if (al) al[j] = alpha_h[j];
            if (be) be[j] = beta_h[j];
        }
        if (h_out) *h_out = h;
        return BROV_OK;
    }
    // the stage alone from `state_in` (null: the stage's own) on `st`, to the host; moves nothing
    int eval_host(const double* commanded, const double* state_in, double* applied_out, double* state_out, const hipStream_t& st, const CallCtx& c) {
        if (!commanded || (!applied_out && !state_out)) return c.refuse("null argument");
        for (size_t j = 0; state_in && j < B * 6; j++)
            if (!std::isfinite(state_in[j])) return c.refuse("the rotor state must be finite");
        if (int rc = ready(c)) return rc;
        const size_t n = B * 6;
        BROV_HIPCHK(c.err, hipMemcpy(eval, commanded, n * sizeof(double), hipMemcpyHostToDevice));
        if (state_in) BROV_HIPCHK(c.err, hipMemcpy(eval + n, state_in, n * sizeof(double), hipMemcpyHostToDevice));
        launch_rotor_eval(par, alpha, beta, eval, state_in ? eval + n : state, eval + 2 * n, eval + 3 * n, (int)B, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        if (applied_out) BROV_HIPCHK(c.err, hipMemcpy(applied_out, eval + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost));
        if (state_out) BROV_HIPCHK(c.err, hipMemcpy(state_out, eval + 3 * n, n * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int last_seconds(double* seconds, const CallCtx& c) { return PlantStage::last_seconds(seconds, "no plant step behind the rotor stage yet", c); }
};

}  // namespace brov
