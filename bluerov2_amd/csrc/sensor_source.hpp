// sensor_source.hpp -- the host side of the sensor stage (sensor_kernel.hip: sensor_measure_kernel, sensor_eval_kernel; the public names are
// brov_sensor_* of include/bluerov2_nmpc.h): the configuration in force, its device buffers, the measured state, the statistics of the
// regular refreshes and the timing of the last refresh.  Its owner is a brov_solver, whose entry points check their own handle and forward here
// with the owner's wait for what may still read or write the buffers (Wait: it selects the device, waits on the host and returns a code), which
// is called once the arguments have passed: a refused call changes nothing and waits for nothing.
// Host code only, header only; what reports takes the string to write and the caller's name, the convention of host_common.hpp.
#pragma once
#include <cmath>
#include <functional>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

struct SensorSource {
    static constexpr long long kSensorMaxIndex = 1LL << 24;   // the measurement index has 24 bits of the noise counter
    bool on = false;               // the solve, the observer and the estimator read ymeas (off: the plant's state, as they always did)
    bool configured = false;       // the buffers hold a configuration (the last brov_sensor_set_host's, or the defaults)
    size_t B = 0;                  // instances, set by the owner at create
    SensorPar par{};               // quant, period, seed in force
    SensorDev dev;                 // sigma, bias, dropout and the statistics: from the owner's DeviceAllocs, on first use
    double *sigma = nullptr, *bias = nullptr, *dropout = nullptr;   // (the writable ends of dev's pointers)
    double* eval = nullptr;        // [2][B][12] of eval_host
    int32_t* eval_drop = nullptr;  // [B] ...
    double* ymeas = nullptr;       // [B][12] the measured state (zeros before the first refresh)
    long long refreshes = 0;       // regular refreshes since the statistics were reset
    KernelTimer timer;             // around the measure kernel's last launch

    using Wait = std::function<int()>;

    void destroy() { timer.destroy(); }

    // is `m` a measurement index the counter can hold?
    static int index_ok(long long m, std::string& err, const char* who) {
        if (m < 0 || m >= kSensorMaxIndex) {
            err = std::string(who) + ": the sensor stage's measurement index (the plant's tick counter) must stay in [0, 2^24)";
            return BROV_ERR_ARG;
        }
        return BROV_OK;
    }
    // with the stage on: may the counter, now at `tick`, move on `n` plant steps?  The last refresh is at tick + n
    int steps_ok(long long tick, long long n, std::string& err, const char* who) const {
        return on && n > 0 ? index_ok(tick + n, err, who) : BROV_OK;
    }

    int allocate(DeviceAllocs& mem, std::string& err) {
        if (ymeas) return BROV_OK;   // (allocated last: it marks the set as complete)
        if (!sigma) { if (int rc = mem.alloc(&sigma, B * 12, err)) return rc; }
        if (!bias) { if (int rc = mem.alloc(&bias, B * 12, err)) return rc; }
        if (!dropout) { if (int rc = mem.alloc(&dropout, B, err)) return rc; }
        if (!eval) { if (int rc = mem.alloc(&eval, 2 * B * 12, err)) return rc; }
        if (!eval_drop) { if (int rc = mem.alloc(&eval_drop, B, err)) return rc; }
        if (!dev.dropped) { if (int rc = mem.alloc(&dev.dropped, B, err)) return rc; }
        if (!dev.err_sq) { if (int rc = mem.alloc(&dev.err_sq, B * 12, err)) return rc; }
        if (!timer.ev[0]) BROV_HIPCHK(err, timer.create());
        BROV_HIPCHK(err, hipMemset(dev.dropped, 0, B * sizeof(int32_t)));
        BROV_HIPCHK(err, hipMemset(dev.err_sq, 0, B * 12 * sizeof(double)));
        double* y = nullptr;
        if (int rc = mem.alloc(&y, B * 12, err)) return rc;
        BROV_HIPCHK(err, hipMemset(y, 0, B * 12 * sizeof(double)));
        dev.sigma = sigma; dev.bias = bias; dev.dropout = dropout; ymeas = y;
        return BROV_OK;
    }
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
    int reset_stats(const Wait& wait, DeviceAllocs& mem, std::string& err) {
        if (int rc = wait()) return rc;
        if (int rc = allocate(mem, err)) return rc;
        BROV_HIPCHK(err, hipMemset(dev.dropped, 0, B * sizeof(int32_t)));
        BROV_HIPCHK(err, hipMemset(dev.err_sq, 0, B * 12 * sizeof(double)));
        refreshes = 0;
        return BROV_OK;
    }
    // buffers and a configuration for a call that reads them before any brov_sensor_set_host: the defaults, the stage stays off
    int ensure(DeviceAllocs& mem, std::string& err) {
        if (int rc = allocate(mem, err)) return rc;
        return configured ? BROV_OK : upload(0, nullptr, nullptr, nullptr, nullptr, nullptr, err);
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
                 const double* x, long long m, hipStream_t st, const Wait& wait, DeviceAllocs& mem, std::string& err, const char* who) {
        for (size_t j = 0; sigma_h && j < B * 12; j++)
            if (!(sigma_h[j] >= 0.0)) { err = std::string(who) + ": sigma must be >= 0 (and not NaN)"; return BROV_ERR_ARG; }
        for (size_t j = 0; bias_h && j < B * 12; j++)
            if (!std::isfinite(bias_h[j])) { err = std::string(who) + ": bias must be finite"; return BROV_ERR_ARG; }
        for (int c = 0; c < 12; c++) {
            if (quant && !(quant[c] >= 0.0)) { err = std::string(who) + ": quant must be >= 0 (and not NaN; 0: none)"; return BROV_ERR_ARG; }
            if (period && period[c] < 1) { err = std::string(who) + ": period must be >= 1"; return BROV_ERR_ARG; }
        }
        for (size_t b = 0; dropout_h && b < B; b++)
            if (!(dropout_h[b] >= 0.0 && dropout_h[b] <= 1.0)) { err = std::string(who) + ": dropout must lie in [0, 1]"; return BROV_ERR_ARG; }
        if (int rc = index_ok(m, err, who)) return rc;
        if (int rc = reset_stats(wait, mem, err)) return rc;
        if (int rc = upload(seed, sigma_h, bias_h, quant, period, dropout_h, err)) return rc;
        on = true;
        measure(x, m, true, st);
        BROV_HIPCHK(err, hipGetLastError());
        return BROV_OK;
    }
    int set_off() { on = false; return BROV_OK; }

    // the stage alone at index `m` on `st`, to the host; moves nothing and touches no statistic
    int eval_host(int64_t m, const double* x, double* y, int32_t* dropped, const hipStream_t& st, const Wait& wait, DeviceAllocs& mem,
                  std::string& err, const char* who) {
        if (!x || !y) { err = std::string(who) + ": null argument"; return BROV_ERR_ARG; }
        if (int rc = index_ok((long long)m, err, who)) return rc;
        if (int rc = wait()) return rc;
        if (int rc = ensure(mem, err)) return rc;
        const size_t n = B * 12;
        BROV_HIPCHK(err, hipMemcpy(eval, x, n * sizeof(double), hipMemcpyHostToDevice));
        launch_sensor_eval(par, dev, (int)B, (long long)m, eval, eval + n, eval_drop, st);
        BROV_HIPCHK(err, hipGetLastError());
        BROV_HIPCHK(err, hipStreamSynchronize(st));
        BROV_HIPCHK(err, hipMemcpy(y, eval + n, n * sizeof(double), hipMemcpyDeviceToHost));
        if (dropped) BROV_HIPCHK(err, hipMemcpy(dropped, eval_drop, B * sizeof(int32_t), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_measurement_host(double* y, const Wait& wait, DeviceAllocs& mem, std::string& err, const char* who) {
        if (!y) { err = std::string(who) + ": null argument"; return BROV_ERR_ARG; }
        if (int rc = wait()) return rc;
        if (int rc = ensure(mem, err)) return rc;
        BROV_HIPCHK(err, hipMemcpy(y, ymeas, B * 12 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_stats_host(int32_t* dropped, double* err_sq, int64_t* refreshes_out, const Wait& wait, DeviceAllocs& mem, std::string& err) {
        if (int rc = wait()) return rc;
        if (int rc = ensure(mem, err)) return rc;
        if (dropped) BROV_HIPCHK(err, hipMemcpy(dropped, dev.dropped, B * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (err_sq) BROV_HIPCHK(err, hipMemcpy(err_sq, dev.err_sq, B * 12 * sizeof(double), hipMemcpyDeviceToHost));
        if (refreshes_out) *refreshes_out = (int64_t)refreshes;
        return BROV_OK;
    }
    int last_seconds(double* seconds, std::string& err, const char* who) {
        if (!seconds) { err = std::string(who) + ": null argument"; return BROV_ERR_ARG; }
        if (!timer.valid) { err = std::string(who) + ": no refresh of the measured state yet"; return BROV_ERR_ARG; }
        return timer.seconds(seconds, err);
    }
};

}  // namespace brov
