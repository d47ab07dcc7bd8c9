// thruster_source.hpp -- the host side of the plant's thruster stage (plant_wrench.hip: thruster_eval_kernel, plant_thruster_kernel; the
// public names are brov_thruster_* of include/bluerov2_nmpc.h): the configuration in force, its device buffers, the statistics of the plant
// steps and the timing of the last one.  Its owner is a brov_solver, whose entry points check their own handle and forward here with the
// owner's wait for what may still read or write the buffers (Wait: it selects the device, waits on the host and returns a code), which is
// called once the arguments have passed: a refused call changes nothing and waits for nothing.
// Host code only, header only; what reports takes the string to write and the caller's name, the convention of host_common.hpp.
#pragma once
#include <cmath>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

struct ThrusterSource {
    bool on = false;               // the plant steps run behind the stage (off: the plant kernels as they always were)
    bool configured = false;       // the buffers hold a configuration (the last brov_thruster_set_host's, or the defaults)
    size_t B = 0;                  // instances, set by the owner at create
    ThrusterPar par;               // K, lo, hi in force
    ThrusterDev dev;               // gain, bias, onset, statistics and last applied thrusts: from the owner's DeviceAllocs, on first use
    double *gain = nullptr, *bias = nullptr, *eval = nullptr;   // (the writable ends of dev's pointers; eval: [3][B][6] of eval_host)
    long long* onset = nullptr;
    long long steps = 0;           // plant steps behind the stage since the statistics were reset
    KernelTimer timer;             // around the plant kernel's last launch

    using Wait = std::function<int()>;

    // the model's own propulsion matrix: rows 0, 1, 2, 5 as make_wrench (bluerov2_model.hpp) has them, rows 3, 4 zero
    static void default_matrix(double K[36]) {
        static const double M[36] = {0.707, 0.707, -0.707, -0.707, 0, 0, 0.707, -0.707, 0.707, -0.707, 0, 0, 0, 0, 0, 0, 1, 1,
                                     0,     0,     0,      0,      0, 0, 0,     0,      0,     0,      0, 0, 0.167, -0.167, -0.175, 0.175, 0, 0};
        for (int j = 0; j < 36; j++) K[j] = M[j];
    }
    void destroy() { timer.destroy(); }

    int allocate(DeviceAllocs& mem, std::string& err) {
        if (dev.last) return BROV_OK;   // (allocated last: it marks the set as complete)
        if (!gain) { if (int rc = mem.alloc(&gain, B * 6, err)) return rc; }
        if (!bias) { if (int rc = mem.alloc(&bias, B * 6, err)) return rc; }
        if (!onset) { if (int rc = mem.alloc(&onset, B, err)) return rc; }
        if (!eval) { if (int rc = mem.alloc(&eval, 3 * B * 6, err)) return rc; }
        if (!dev.clip_ticks) { if (int rc = mem.alloc(&dev.clip_ticks, B * 6, err)) return rc; }
        if (!dev.lost_sq) { if (int rc = mem.alloc(&dev.lost_sq, B, err)) return rc; }
        if (!timer.ev[0]) BROV_HIPCHK(err, timer.create());
        BROV_HIPCHK(err, hipMemset(dev.clip_ticks, 0, B * 6 * sizeof(int32_t)));
        BROV_HIPCHK(err, hipMemset(dev.lost_sq, 0, B * sizeof(double)));
        double* last = nullptr;
        if (int rc = mem.alloc(&last, B * 6, err)) return rc;
        BROV_HIPCHK(err, hipMemset(last, 0, B * 6 * sizeof(double)));
        dev.gain = gain; dev.bias = bias; dev.onset = onset; dev.last = last;
        return BROV_OK;
    }
    // the configuration into the buffers (NULL: the default of that argument); the caller has waited
    int upload(const double* K, const double* lo, const double* hi, const double* gain_h, const double* bias_h, const int64_t* onset_h,
               std::string& err) {
        const double inf = std::numeric_limits<double>::infinity();
        std::vector<double> fill(B * 6);
        std::fill(fill.begin(), fill.end(), 1.0);
        BROV_HIPCHK(err, hipMemcpy(gain, gain_h ? gain_h : fill.data(), B * 6 * sizeof(double), hipMemcpyHostToDevice));
        std::fill(fill.begin(), fill.end(), 0.0);
        BROV_HIPCHK(err, hipMemcpy(bias, bias_h ? bias_h : fill.data(), B * 6 * sizeof(double), hipMemcpyHostToDevice));
        if (onset_h) {
            std::vector<long long> on64(onset_h, onset_h + B);
            BROV_HIPCHK(err, hipMemcpy(onset, on64.data(), B * sizeof(long long), hipMemcpyHostToDevice));
        } else {
            BROV_HIPCHK(err, hipMemset(onset, 0, B * sizeof(long long)));
        }
        if (K) for (int j = 0; j < 36; j++) par.K[j] = K[j];
        else default_matrix(par.K);
        for (int i = 0; i < 6; i++) { par.lo[i] = lo ? lo[i] : -inf; par.hi[i] = hi ? hi[i] : inf; }
        configured = true;
        return BROV_OK;
    }
    int reset_stats(const Wait& wait, DeviceAllocs& mem, std::string& err) {
        if (int rc = wait()) return rc;
        if (int rc = allocate(mem, err)) return rc;
        BROV_HIPCHK(err, hipMemset(dev.clip_ticks, 0, B * 6 * sizeof(int32_t)));
        BROV_HIPCHK(err, hipMemset(dev.lost_sq, 0, B * sizeof(double)));
        steps = 0;
        return BROV_OK;
    }
    // buffers and a configuration for a call that reads them before any brov_thruster_set_host: the defaults, the stage stays off
    int ensure(DeviceAllocs& mem, std::string& err) {
        if (int rc = allocate(mem, err)) return rc;
        return configured ? BROV_OK : upload(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, err);
    }

    int set_host(const double* K, const double* lo, const double* hi, const double* gain_h, const double* bias_h, const int64_t* onset_h,
                 const Wait& wait, DeviceAllocs& mem, std::string& err, const char* who) {
        auto finite = [](const double* v, size_t n) {
            for (size_t j = 0; v && j < n; j++) if (!std::isfinite(v[j])) return false;
            return true;
        };
        for (int i = 0; i < 6; i++) {
            const double l = lo ? lo[i] : -1.0, h = hi ? hi[i] : 1.0;
            if (std::isnan(l) || std::isnan(h)) { err = std::string(who) + ": a thrust limit is NaN"; return BROV_ERR_ARG; }
            if (lo && hi && l > h) { err = std::string(who) + ": lo[i] > hi[i]: a thrust limit pair is empty"; return BROV_ERR_ARG; }
        }
        if (!finite(K, 36) || !finite(gain_h, B * 6) || !finite(bias_h, B * 6)) {
            err = std::string(who) + ": K, gain and bias must be finite";
            return BROV_ERR_ARG;
        }
        for (size_t b = 0; onset_h && b < B; b++)
            if (onset_h[b] < 0) { err = std::string(who) + ": negative onset tick"; return BROV_ERR_ARG; }
        if (int rc = reset_stats(wait, mem, err)) return rc;
        if (int rc = upload(K, lo, hi, gain_h, bias_h, onset_h, err)) return rc;
        on = true;
        return BROV_OK;
    }
    int set_off() { on = false; return BROV_OK; }

    // the stage alone at tick `t` on `st`, to the host; moves no counter and touches no statistic
    int eval_host(int64_t t, const double* commanded, double* applied, double* wrench, const hipStream_t& st, const Wait& wait, DeviceAllocs& mem,
                  std::string& err, const char* who) {
        if (!commanded || !applied || !wrench) { err = std::string(who) + ": null argument"; return BROV_ERR_ARG; }
        if (t < 0) { err = std::string(who) + ": negative tick"; return BROV_ERR_ARG; }
        if (int rc = wait()) return rc;
        if (int rc = ensure(mem, err)) return rc;
        const size_t n = B * 6;
        BROV_HIPCHK(err, hipMemcpy(eval, commanded, n * sizeof(double), hipMemcpyHostToDevice));
        launch_thruster_eval(par, dev, (int)B, (long long)t, eval, eval + n, eval + 2 * n, st);
        BROV_HIPCHK(err, hipGetLastError());
        BROV_HIPCHK(err, hipStreamSynchronize(st));
        BROV_HIPCHK(err, hipMemcpy(applied, eval + n, n * sizeof(double), hipMemcpyDeviceToHost));
        BROV_HIPCHK(err, hipMemcpy(wrench, eval + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int last_host(double* applied, const Wait& wait, DeviceAllocs& mem, std::string& err, const char* who) {
        if (!applied) { err = std::string(who) + ": null argument"; return BROV_ERR_ARG; }
        if (int rc = wait()) return rc;
        if (int rc = ensure(mem, err)) return rc;
        BROV_HIPCHK(err, hipMemcpy(applied, dev.last, B * 6 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_stats_host(int32_t* clip_ticks, double* lost_sq, int64_t* steps_out, const Wait& wait, DeviceAllocs& mem, std::string& err) {
        if (int rc = wait()) return rc;
        if (int rc = ensure(mem, err)) return rc;
        if (clip_ticks) BROV_HIPCHK(err, hipMemcpy(clip_ticks, dev.clip_ticks, B * 6 * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (lost_sq) BROV_HIPCHK(err, hipMemcpy(lost_sq, dev.lost_sq, B * sizeof(double), hipMemcpyDeviceToHost));
        if (steps_out) *steps_out = (int64_t)steps;
        return BROV_OK;
    }
    int last_seconds(double* seconds, std::string& err, const char* who) {
        if (!seconds) { err = std::string(who) + ": null argument"; return BROV_ERR_ARG; }
        if (!timer.valid) { err = std::string(who) + ": no plant step behind the thruster stage yet"; return BROV_ERR_ARG; }
        return timer.seconds(seconds, err);
    }

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
