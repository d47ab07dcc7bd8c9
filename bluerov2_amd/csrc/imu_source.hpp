// imu_source.hpp -- the host side of the IMU/GPS stage (imu_kernel.hip: imu_measure_kernel, imu_eval_kernel; the public names are brov_imu_* of
// include/bluerov2_nmpc_imu.h): the configuration in force, its device buffers, the last sample with its fix flags, the stage's own state
// (v_I of the last sample, the last fix and its index), the statistics of the regular refreshes and the timing of the last refresh.  Its
// owner is a brov_solver, whose entry points check their own handle and forward here with the owner's call context (CallCtx, host_common.hpp)
// as they do for the sensor stage, whose shape this follows.  The stage always reads the TRUE plant state: it is the sensor.  Host code only,
// header only.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

struct ImuSource : PlantStage {
    static constexpr long long kImuMaxIndex = 1LL << 24;   // the measurement index has 24 bits of the noise counter
    ImuPar par{0.0, 9.81, 1, 0, 0};   // h, g, gps_every, flags, seed in force
    ImuDev dev;                    // sigma, bias, dropout, the stage's state and the statistics: from the owner's DeviceAllocs, on first use
    ImuOut out{};                  // the last sample: imu [B][6], gps_p [B][3], gps_v [B][3], q_meas [B][4], fix [B] (zeros before the first)
    double *sigma = nullptr, *bias = nullptr, *dropout = nullptr;   // (the writable ends of dev's pointers)
    double* eval = nullptr;        // [B][12 + 3 + 3] of eval_host: x, v_prev, gps_p_last ...
    int32_t* eval_m = nullptr;     // [B] ... m_last
    ImuOut eval_out{};             // ... and its sample
    long long refreshes = 0;       // regular refreshes since the statistics were reset
    bool fix_due = false;          // the last refresh was one at which a fix was due (a forced one always is): some fix[b] may be 1

    static int index_ok(long long m, const CallCtx& c) {
        if (m < 0 || m >= kImuMaxIndex) return c.refuse("the IMU stage's measurement index (the plant's tick counter) must stay in [0, 2^24)");
        return BROV_OK;
    }
    // with the stage on: may the counter, now at `tick`, move on `n` plant steps?  The last refresh is at tick + n
    int steps_ok(long long tick, long long n, const CallCtx& c) const { return on && n > 0 ? index_ok(tick + n, c) : BROV_OK; }
    // with the stage on: a plant step of length `dt`?  The acceleration is differenced over h, the fixes are timed in steps of h
    int dt_ok(double dt, const CallCtx& c) const {
        return on && dt != par.h ? c.refuse("the IMU stage is on and dt is not the step h it samples (brov_imu_set_host)") : BROV_OK;
    }

    int out_buffers(ImuOut& o, const CallCtx& c) {
        if (int rc = buffer(&o.imu, B * 6, c)) return rc;
        if (int rc = buffer(&o.gps_p, B * 3, c)) return rc;
        if (int rc = buffer(&o.gps_v, B * 3, c)) return rc;
        if (int rc = buffer(&o.qm, B * 4, c)) return rc;
        return buffer(&o.fix, B, c);
    }
    // the buffers on first use, and a configuration for a call that reads them before any brov_imu_set_host: the defaults, the stage stays off
    int ensure(const CallCtx& c) {
        if (int rc = buffer(&sigma, B * 12, c)) return rc;
        if (int rc = buffer(&bias, B * 6, c)) return rc;
        if (int rc = buffer(&dropout, B, c)) return rc;
        if (int rc = buffer(&dev.vprev, B * 3, c)) return rc;
        if (int rc = buffer(&dev.plast, B * 3, c)) return rc;
        if (int rc = buffer(&dev.mlast, B, c)) return rc;
        if (int rc = buffer(&dev.stats, B * 3, c)) return rc;
        if (int rc = buffer(&eval, B * 18, c)) return rc;
        if (int rc = buffer(&eval_m, B, c)) return rc;
        if (int rc = out_buffers(out, c)) return rc;
        if (int rc = out_buffers(eval_out, c)) return rc;
        dev.sigma = sigma; dev.bias = bias; dev.dropout = dropout;
        return configured ? BROV_OK : upload(nullptr, nullptr, nullptr, c.err);
    }
    int ready(const CallCtx& c) { const int rc = c.wait(); return rc ? rc : ensure(c); }
    // the per-instance configuration into the buffers (NULL: zeros); the caller has waited
    int upload(const double* sigma_h, const double* bias_h, const double* dropout_h, std::string& err) {
        const std::vector<double> zeros(B * 12, 0.0);
        BROV_HIPCHK(err, hipMemcpy(sigma, sigma_h ? sigma_h : zeros.data(), B * 12 * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(err, hipMemcpy(bias, bias_h ? bias_h : zeros.data(), B * 6 * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(err, hipMemcpy(dropout, dropout_h ? dropout_h : zeros.data(), B * sizeof(double), hipMemcpyHostToDevice));
        configured = true;
        return BROV_OK;
    }
    int reset_stats(const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemset(dev.stats, 0, B * 3 * sizeof(int32_t)));
        refreshes = 0;
        return BROV_OK;
    }

    // one refresh from the true state `x` at index `m` on `st` (the owner has checked `on` and the index), timed
    void measure(const double* x, long long m, bool forced, hipStream_t st) {
        (void)timer.start(st);
        launch_imu_measure(par, dev, out, (int)B, m, forced, x, st);
        (void)timer.stop(st);
        fix_due = forced || m % par.gps_every == 0;
        if (!forced) refreshes++;
    }

    // the configuration comes into force, the statistics start afresh and the stage restarts (a forced refresh) from `x` at index `m` on `st`
    int set_host(const brov_imu_params* p, const double* sigma_h, const double* bias_h, const double* dropout_h, const double* x, long long m,
                 hipStream_t st, const CallCtx& c) {
        if (!p) return c.refuse("null argument");
        if (!(p->h > 0.0) || !std::isfinite(p->h)) return c.refuse("h must be positive");
        if (!(p->g >= 0.0) || !std::isfinite(p->g)) return c.refuse("g must be finite and >= 0");
        if (p->gps_every < 1) return c.refuse("gps_every must be >= 1");
        if (p->flags & ~BROV_IMU_GPSV_ELAPSED) return c.refuse("unknown flag");
        for (size_t j = 0; sigma_h && j < B * 12; j++)
            if (!(sigma_h[j] >= 0.0)) return c.refuse("sigma must be >= 0 (and not NaN)");
        for (size_t j = 0; bias_h && j < B * 6; j++)
            if (!std::isfinite(bias_h[j])) return c.refuse("bias must be finite");
        for (size_t b = 0; dropout_h && b < B; b++)
            if (!(dropout_h[b] >= 0.0 && dropout_h[b] <= 1.0)) return c.refuse("dropout must lie in [0, 1]");
        if (int rc = index_ok(m, c)) return rc;
        if (int rc = reset_stats(c)) return rc;
        if (int rc = upload(sigma_h, bias_h, dropout_h, c.err)) return rc;
        par.h = p->h; par.g = p->g; par.gps_every = p->gps_every; par.flags = p->flags; par.seed = p->seed;
        on = true;
        measure(x, m, true, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        return BROV_OK;
    }

    // the stage alone at index `m` on `st`, to the host; moves nothing and touches no statistic
    int eval_host(int64_t m, const double* x, const double* v_prev, const double* gps_p_last, const int32_t* m_last, double* imu, double* gps_p,
                  double* gps_v, double* q_meas, int32_t* fix, const hipStream_t& st, const CallCtx& c) {
        if (!x || !v_prev || !gps_p_last || !m_last) return c.refuse("null argument");
        if (int rc = index_ok((long long)m, c)) return rc;
        if (int rc = ready(c)) return rc;
        double *xd = eval, *vd = eval + B * 12, *pd = eval + B * 15;
        BROV_HIPCHK(c.err, hipMemcpy(xd, x, B * 12 * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(c.err, hipMemcpy(vd, v_prev, B * 3 * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(c.err, hipMemcpy(pd, gps_p_last, B * 3 * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(c.err, hipMemcpy(eval_m, m_last, B * sizeof(int32_t), hipMemcpyHostToDevice));
        BROV_HIPCHK(c.err, hipMemset(eval_out.gps_p, 0, B * 3 * sizeof(double)));   // without a fix: zeros
        BROV_HIPCHK(c.err, hipMemset(eval_out.gps_v, 0, B * 3 * sizeof(double)));
        BROV_HIPCHK(c.err, hipMemset(eval_out.qm, 0, B * 4 * sizeof(double)));
        launch_imu_eval(par, dev, eval_out, (int)B, (long long)m, xd, vd, pd, eval_m, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        return get(eval_out, imu, gps_p, gps_v, q_meas, fix, c.err);
    }
    int get(const ImuOut& o, double* imu, double* gps_p, double* gps_v, double* q_meas, int32_t* fix, std::string& err) const {
        if (imu) BROV_HIPCHK(err, hipMemcpy(imu, o.imu, B * 6 * sizeof(double), hipMemcpyDeviceToHost));
        if (gps_p) BROV_HIPCHK(err, hipMemcpy(gps_p, o.gps_p, B * 3 * sizeof(double), hipMemcpyDeviceToHost));
        if (gps_v) BROV_HIPCHK(err, hipMemcpy(gps_v, o.gps_v, B * 3 * sizeof(double), hipMemcpyDeviceToHost));
        if (q_meas) BROV_HIPCHK(err, hipMemcpy(q_meas, o.qm, B * 4 * sizeof(double), hipMemcpyDeviceToHost));
        if (fix) BROV_HIPCHK(err, hipMemcpy(fix, o.fix, B * sizeof(int32_t), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_host(double* imu, double* gps_p, double* gps_v, double* q_meas, int32_t* fix, const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        return get(out, imu, gps_p, gps_v, q_meas, fix, c.err);
    }
    int get_stats_host(int32_t* stats, int64_t* refreshes_out, const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        if (stats) BROV_HIPCHK(c.err, hipMemcpy(stats, dev.stats, B * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (refreshes_out) *refreshes_out = (int64_t)refreshes;
        return BROV_OK;
    }
    int last_seconds(double* seconds, const CallCtx& c) { return PlantStage::last_seconds(seconds, "no refresh of the IMU stage yet", c); }
};

}  // namespace brov
