// thruster_source.hpp -- the host side of the plant's thruster stage (plant_wrench.hip: thruster_eval_kernel, plant_thruster_kernel; the
// public names are brov_thruster_* of include/bluerov2_nmpc.h): the configuration in force, its device buffers, the statistics of the plant
// steps and the timing of the last one.  Its owner is a brov_solver, whose entry points check their own handle and forward here with the
// owner's call context (CallCtx, host_common.hpp): its wait, for what may still read or write the buffers, is called once the arguments have
// passed, so a refused call changes nothing and waits for nothing.  Shares PlantStage with the sensor stage.  Host code only, header only.
#pragma once
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

struct ThrusterSource : PlantStage {   // on: the plant steps run behind the stage (off: the plant kernels as they always were)
    ThrusterPar par;               // K, lo, hi in force
    ThrusterDev dev;               // gain, bias, onset, statistics and last applied thrusts: from the owner's DeviceAllocs, on first use
    double *gain = nullptr, *bias = nullptr, *eval = nullptr;   // (the writable ends of dev's pointers; eval: [3][B][6] of eval_host)
    long long* onset = nullptr;
    long long steps = 0;           // plant steps behind the stage since the statistics were reset

    // the model's own propulsion matrix: rows 0, 1, 2, 5 as make_wrench (bluerov2_model.hpp) has them, rows 3, 4 zero
    static void default_matrix(double K[36]) {
        static const double M[36] = {0.707, 0.707, -0.707, -0.707, 0, 0, 0.707, -0.707, 0.707, -0.707, 0, 0, 0, 0, 0, 0, 1, 1,
                                     0,     0,     0,      0,      0, 0, 0,     0,      0,     0,      0, 0, 0.167, -0.167, -0.175, 0.175, 0, 0};
        for (int j = 0; j < 36; j++) K[j] = M[j];
    }

    // the buffers on first use, and a configuration for a call that reads them before any brov_thruster_set_host: the defaults, the stage stays off
    int ensure(const CallCtx& c) {
        if (int rc = buffer(&gain, B * 6, c)) return rc;
        if (int rc = buffer(&bias, B * 6, c)) return rc;
        if (int rc = buffer(&onset, B, c)) return rc;
        if (int rc = buffer(&eval, 3 * B * 6, c)) return rc;
        if (int rc = buffer(&dev.clip_ticks, B * 6, c)) return rc;
        if (int rc = buffer(&dev.lost_sq, B, c)) return rc;
        if (int rc = buffer(&dev.last, B * 6, c)) return rc;
        dev.gain = gain; dev.bias = bias; dev.onset = onset;
        return configured ? BROV_OK : upload(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c.err);
    }
    // ... behind the owner's wait: what every call that reads or writes the buffers begins with once its arguments have passed
    int ready(const CallCtx& c) { const int rc = c.wait(); return rc ? rc : ensure(c); }
    // the configuration into the buffers (NULL: the default of that argument); the caller has waited
    int upload(const double* K, const double* lo, const double* hi, const double* gain_h, const double* bias_h, const int64_t* onset_h,
               std::string& err) {
        const double inf = std::numeric_limits<double>::infinity();
        const std::vector<double> ones(B * 6, 1.0), zeros(B * 6, 0.0);
        BROV_HIPCHK(err, hipMemcpy(gain, gain_h ? gain_h : ones.data(), B * 6 * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(err, hipMemcpy(bias, bias_h ? bias_h : zeros.data(), B * 6 * sizeof(double), hipMemcpyHostToDevice));
        static_assert(sizeof(long long) == sizeof(int64_t), "the device's onset ticks are the caller's, copied as they are");
        if (onset_h) BROV_HIPCHK(err, hipMemcpy(onset, onset_h, B * sizeof(int64_t), hipMemcpyHostToDevice));
        else BROV_HIPCHK(err, hipMemset(onset, 0, B * sizeof(int64_t)));
        if (K) for (int j = 0; j < 36; j++) par.K[j] = K[j];
        else default_matrix(par.K);
        for (int i = 0; i < 6; i++) { par.lo[i] = lo ? lo[i] : -inf; par.hi[i] = hi ? hi[i] : inf; }
        configured = true;
        return BROV_OK;
    }
    int reset_stats(const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemset(dev.clip_ticks, 0, B * 6 * sizeof(int32_t)));
        BROV_HIPCHK(c.err, hipMemset(dev.lost_sq, 0, B * sizeof(double)));
        steps = 0;
        return BROV_OK;
    }

    int set_host(const double* K, const double* lo, const double* hi, const double* gain_h, const double* bias_h, const int64_t* onset_h,
                 const CallCtx& c) {
        auto finite = [](const double* v, size_t n) {
            for (size_t j = 0; v && j < n; j++) if (!std::isfinite(v[j])) return false;
            return true;
        };
        for (int i = 0; i < 6; i++) {
            const double l = lo ? lo[i] : -1.0, h = hi ? hi[i] : 1.0;
            if (std::isnan(l) || std::isnan(h)) return c.refuse("a thrust limit is NaN");
            if (lo && hi && l > h) return c.refuse("lo[i] > hi[i]: a thrust limit pair is empty");
        }
        if (!finite(K, 36) || !finite(gain_h, B * 6) || !finite(bias_h, B * 6)) return c.refuse("K, gain and bias must be finite");
        for (size_t b = 0; onset_h && b < B; b++)
            if (onset_h[b] < 0) return c.refuse("negative onset tick");
        if (int rc = reset_stats(c)) return rc;
        if (int rc = upload(K, lo, hi, gain_h, bias_h, onset_h, c.err)) return rc;
        on = true;
        return BROV_OK;
    }

    // the stage alone at tick `t` on `st`, to the host; moves no counter and touches no statistic
    int eval_host(int64_t t, const double* commanded, double* applied, double* wrench, const hipStream_t& st, const CallCtx& c) {
        if (!commanded || !applied || !wrench) return c.refuse("null argument");
        if (t < 0) return c.refuse("negative tick");
        if (int rc = ready(c)) return rc;
        const size_t n = B * 6;
        BROV_HIPCHK(c.err, hipMemcpy(eval, commanded, n * sizeof(double), hipMemcpyHostToDevice));
        launch_thruster_eval(par, dev, (int)B, (long long)t, eval, eval + n, eval + 2 * n, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        BROV_HIPCHK(c.err, hipMemcpy(applied, eval + n, n * sizeof(double), hipMemcpyDeviceToHost));
        BROV_HIPCHK(c.err, hipMemcpy(wrench, eval + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int last_host(double* applied, const CallCtx& c) {
        if (!applied) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(applied, dev.last, B * 6 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_stats_host(int32_t* clip_ticks, double* lost_sq, int64_t* steps_out, const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        if (clip_ticks) BROV_HIPCHK(c.err, hipMemcpy(clip_ticks, dev.clip_ticks, B * 6 * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (lost_sq) BROV_HIPCHK(c.err, hipMemcpy(lost_sq, dev.lost_sq, B * sizeof(double), hipMemcpyDeviceToHost));
        if (steps_out) *steps_out = (int64_t)steps;
        return BROV_OK;
    }
    int last_seconds(double* seconds, const CallCtx& c) { return PlantStage::last_seconds(seconds, "no plant step behind the thruster stage yet", c); }

    // one plant step behind the stage on `st` (the owner has checked `on`), timed; g.mode OFF: no world wrench on top
    void step(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, double dt, int substeps, double* xlog,
              double* ulog, const WrenchGen& g, long long tick, double* wlog, hipStream_t st) {
        (void)timer.start(st);
        launch_plant_thruster(x0, res, pplant, prp, rp_stride, (int)B, dt, substeps, xlog, ulog, par, dev, g, tick, wlog, st);
        (void)timer.stop(st);
        steps++;
    }
};

}  // namespace brov
