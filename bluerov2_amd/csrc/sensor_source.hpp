// sensor_source.hpp -- the host side of the sensor stage (sensor_kernel.hip: sensor_measure_kernel, sensor_eval_kernel; the public names are
// brov_sensor_* of include/bluerov2_nmpc.h): the configuration in force, its device buffers, the measured state, the statistics of the
// regular refreshes and the timing of the last refresh.  Its owner is a brov_solver, whose entry points check their own handle and forward here
// with the owner's call context (CallCtx, host_common.hpp): its wait, for what may still read or write the buffers, is called once the arguments
// have passed, so a refused call changes nothing and waits for nothing.  Shares PlantStage with the thruster stage.  Host code only, header only.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

struct SensorSource : PlantStage {   // on: the solve, the observer and the estimator read ymeas (off: the plant's state, as they always did)
    static constexpr long long kSensorMaxIndex = 1LL << 24;   // the measurement index has 24 bits of the noise counter
    SensorPar par{};               // quant, period, seed in force
    SensorDev dev;                 // sigma, bias, dropout and the statistics: from the owner's DeviceAllocs, on first use
    double *sigma = nullptr, *bias = nullptr, *dropout = nullptr;   // (the writable ends of dev's pointers)
    double* eval = nullptr;        // [2][B][12] of eval_host
    int32_t* eval_drop = nullptr;  // [B] ...
    double* ymeas = nullptr;       // [B][12] the measured state (zeros before the first refresh)
    long long refreshes = 0;       // regular refreshes since the statistics were reset

    // is `m` a measurement index the counter can hold?
    static int index_ok(long long m, const CallCtx& c) {
        if (m < 0 || m >= kSensorMaxIndex) return c.refuse("the sensor stage's measurement index (the plant's tick counter) must stay in [0, 2^24)");
        return BROV_OK;
    }
    // with the stage on: may the counter, now at `tick`, move on `n` plant steps?  The last refresh is at tick + n
    int steps_ok(long long tick, long long n, const CallCtx& c) const { return on && n > 0 ? index_ok(tick + n, c) : BROV_OK; }

    // the buffers on first use, and a configuration for a call that reads them before any brov_sensor_set_host: the defaults, the stage stays off
    int ensure(const CallCtx& c) {
        if (int rc = buffer(&sigma, B * 12, c)) return rc;
        if (int rc = buffer(&bias, B * 12, c)) return rc;
        if (int rc = buffer(&dropout, B, c)) return rc;
        if (int rc = buffer(&eval, 2 * B * 12, c)) return rc;
        if (int rc = buffer(&eval_drop, B, c)) return rc;
        if (int rc = buffer(&dev.dropped, B, c)) return rc;
        if (int rc = buffer(&dev.err_sq, B * 12, c)) return rc;
        if (int rc = buffer(&ymeas, B * 12, c)) return rc;
        dev.sigma = sigma; dev.bias = bias; dev.dropout = dropout;
        return configured ? BROV_OK : upload(0, nullptr, nullptr, nullptr, nullptr, nullptr, c.err);
    }
    // ... behind the owner's wait: what every call that reads or writes the buffers begins with once its arguments have passed
    int ready(const CallCtx& c) { const int rc = c.wait(); return rc ? rc : ensure(c); }
    // the configuration into the buffers (NULL: the default of that argument); the caller has waited
    int upload(uint64_t seed, const double* sigma_h, const double* bias_h, const double* quant, const int32_t* period, const double* dropout_h,
               std::string& err) {
        const std::vector<double> zeros(B * 12, 0.0);
        BROV_HIPCHK(err, hipMemcpy(sigma, sigma_h ? sigma_h : zeros.data(), B * 12 * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(err, hipMemcpy(bias, bias_h ? bias_h : zeros.data(), B * 12 * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(err, hipMemcpy(dropout, dropout_h ? dropout_h : zeros.data(), B * sizeof(double), hipMemcpyHostToDevice));
        for (int c = 0; c < 12; c++) { par.quant[c] = quant ? quant[c] : 0.0; par.period[c] = period ? period[c] : 1; }
        par.seed = seed;
        configured = true;
        return BROV_OK;
    }
    int reset_stats(const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemset(dev.dropped, 0, B * sizeof(int32_t)));
        BROV_HIPCHK(c.err, hipMemset(dev.err_sq, 0, B * 12 * sizeof(double)));
        refreshes = 0;
        return BROV_OK;
    }

    // one refresh of ymeas from the true state `x` at index `m` on `st` (the owner has checked `on` and the index), timed
    void measure(const double* x, long long m, bool forced, hipStream_t st) {
        (void)timer.start(st);
        launch_sensor_measure(par, dev, (int)B, m, forced, x, ymeas, st);
        (void)timer.stop(st);
        if (!forced) refreshes++;
    }

    // the configuration comes into force, the statistics start afresh and ymeas is refreshed (forced) from `x` at index `m` on `st`
    int set_host(uint64_t seed, const double* sigma_h, const double* bias_h, const double* quant, const int32_t* period, const double* dropout_h,
                 const double* x, long long m, hipStream_t st, const CallCtx& c) {
        for (size_t j = 0; sigma_h && j < B * 12; j++)
            if (!(sigma_h[j] >= 0.0)) return c.refuse("sigma must be >= 0 (and not NaN)");
        for (size_t j = 0; bias_h && j < B * 12; j++)
            if (!std::isfinite(bias_h[j])) return c.refuse("bias must be finite");
        for (int k = 0; k < 12; k++) {
            if (quant && !(quant[k] >= 0.0)) return c.refuse("quant must be >= 0 (and not NaN; 0: none)");
            if (period && period[k] < 1) return c.refuse("period must be >= 1");
        }
        for (size_t b = 0; dropout_h && b < B; b++)
            if (!(dropout_h[b] >= 0.0 && dropout_h[b] <= 1.0)) return c.refuse("dropout must lie in [0, 1]");
        if (int rc = index_ok(m, c)) return rc;
        if (int rc = reset_stats(c)) return rc;
        if (int rc = upload(seed, sigma_h, bias_h, quant, period, dropout_h, c.err)) return rc;
        on = true;
        measure(x, m, true, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        return BROV_OK;
    }

    // the stage alone at index `m` on `st`, to the host; moves nothing and touches no statistic
    int eval_host(int64_t m, const double* x, double* y, int32_t* dropped, const hipStream_t& st, const CallCtx& c) {
        if (!x || !y) return c.refuse("null argument");
        if (int rc = index_ok((long long)m, c)) return rc;
        if (int rc = ready(c)) return rc;
        const size_t n = B * 12;
        BROV_HIPCHK(c.err, hipMemcpy(eval, x, n * sizeof(double), hipMemcpyHostToDevice));
        launch_sensor_eval(par, dev, (int)B, (long long)m, eval, eval + n, eval_drop, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        BROV_HIPCHK(c.err, hipMemcpy(y, eval + n, n * sizeof(double), hipMemcpyDeviceToHost));
        if (dropped) BROV_HIPCHK(c.err, hipMemcpy(dropped, eval_drop, B * sizeof(int32_t), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_measurement_host(double* y, const CallCtx& c) {
        if (!y) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(y, ymeas, B * 12 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_stats_host(int32_t* dropped, double* err_sq, int64_t* refreshes_out, const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        if (dropped) BROV_HIPCHK(c.err, hipMemcpy(dropped, dev.dropped, B * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (err_sq) BROV_HIPCHK(c.err, hipMemcpy(err_sq, dev.err_sq, B * 12 * sizeof(double), hipMemcpyDeviceToHost));
        if (refreshes_out) *refreshes_out = (int64_t)refreshes;
        return BROV_OK;
    }
    int last_seconds(double* seconds, const CallCtx& c) { return PlantStage::last_seconds(seconds, "no refresh of the measured state yet", c); }
};

}  // namespace brov
