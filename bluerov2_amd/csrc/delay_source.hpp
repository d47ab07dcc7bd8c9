// delay_source.hpp -- the host side of the plant's delay stage (delay_kernel.hip: delay_shift_kernel, delay_predict_kernel; the public names
// are brov_delay_* of include/bluerov2_nmpc.h): the configuration in force, the ring of commanded records and the applied records on the
// device, the stage's own step count, the predicted state the last solve started from and the timing of the last launch of either kernel.
// Its owner is a brov_solver, whose entry points check their own handle and forward here with the owner's call context (CallCtx,
// host_common.hpp): its wait, for what may still read or write the buffers, is called once the arguments have passed, so a refused call
// changes nothing and waits for nothing.  Shares PlantStage with the thruster and the sensor stage.  Host code only, header only.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

// the model the predictor integrates: the controller's own, handed down by the owner per call
struct PredictModel {
    const double* par;   // parameters of instance b at par + b * par_stride (the stage-0 row of the controller's)
    int par_stride;
    const double* rp;    // 6-disturbance variant: its roll / pitch moments at rp + b * rp_stride; else nullptr
    int rp_stride;
};

struct DelaySource : PlantStage {   // on: the plant steps read the applied records (off: the solver's own, as they always did)
    static constexpr int kSlots = BROV_DELAY_MAX + 1;   // the ring is allocated for the deepest queue: [B][D][10] with D <= kSlots
    int32_t* delay = nullptr;      // [B] plant steps between a command and its arrival
    double* ring = nullptr;        // [B][D][10] commanded records u0[4] | thrust[6], slot = step mod D
    brov_result* applied = nullptr;   // [B] what the last plant step was given
    double* xhat = nullptr;        // [B][12] what the last solve started from (comp > 0)
    double* ybuf = nullptr;        // [2][B][12] of predict_host: the state given, the prediction
    int D = 1, comp = 0;           // ring depth max(max_b delay[b], comp) + 1; plant steps the controller predicts ahead, one number for the batch
    double dt_pred = 0.0;          // the predictor's step
    bool observer_applied = false; // brov_ekf_update_from_solver reads the applied records in place of the commanded ones
    long long n = 0;               // steps of the stage since it was set or reset: the ring's index
    bool predicted = false;        // a solve has run the predictor since then: xhat means something
    KernelTimer ptimer;            // around the last launch of the predictor (PlantStage::timer: of the shift)

    void destroy() { ptimer.destroy(); PlantStage::destroy(); }
    bool predicts() const { return on && comp > 0; }
    int ahead() const { return on ? comp : 0; }   // rows the loops' reference windows start ahead of the tick

    int ensure(const CallCtx& c) {
        if (int rc = buffer(&delay, B, c)) return rc;
        if (int rc = buffer(&ring, B * kSlots * 10, c)) return rc;
        if (int rc = buffer(&applied, B, c)) return rc;
        if (int rc = buffer(&xhat, B * 12, c)) return rc;
        if (int rc = buffer(&ybuf, 2 * B * 12, c)) return rc;
        if (!ptimer.ev[0]) BROV_HIPCHK(c.err, ptimer.create());
        configured = true;   // (zeroed buffers are the default configuration: no delay, no prediction, a ring of one slot)
        return BROV_OK;
    }
    int ready(const CallCtx& c) { const int rc = c.wait(); return rc ? rc : ensure(c); }
    // the ring, the applied records and the step count to zero; the caller has waited
    int clear(std::string& err) {
        BROV_HIPCHK(err, hipMemset(ring, 0, B * kSlots * 10 * sizeof(double)));
        BROV_HIPCHK(err, hipMemset(applied, 0, B * sizeof(brov_result)));
        n = 0; predicted = false;
        return BROV_OK;
    }
    int reset(const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        return clear(c.err);
    }

    int set_host(const int32_t* delay_h, int32_t comp_, double dt_pred_, double Ts, int32_t observer_applied_, const CallCtx& c) {
        int dmax = 0;
        for (size_t b = 0; delay_h && b < B; b++) {
            if (delay_h[b] < 0 || delay_h[b] > BROV_DELAY_MAX) return c.refuse("delay must lie in [0, BROV_DELAY_MAX]");
            dmax = delay_h[b] > dmax ? delay_h[b] : dmax;
        }
        if (comp_ < 0 || comp_ > BROV_DELAY_MAX) return c.refuse("comp must lie in [0, BROV_DELAY_MAX]");
        if (!std::isfinite(dt_pred_)) return c.refuse("dt_pred must be finite (<= 0: the options' Ts)");
        if (int rc = ready(c)) return rc;
        if (delay_h) BROV_HIPCHK(c.err, hipMemcpy(delay, delay_h, B * sizeof(int32_t), hipMemcpyHostToDevice));
        else BROV_HIPCHK(c.err, hipMemset(delay, 0, B * sizeof(int32_t)));
        D = (dmax > comp_ ? dmax : comp_) + 1;
        comp = comp_; dt_pred = dt_pred_ > 0.0 ? dt_pred_ : Ts; observer_applied = observer_applied_ != 0;
        if (int rc = clear(c.err)) return rc;
        on = true;
        return BROV_OK;
    }

    // one step of the stage on `st` ahead of the plant kernel (the owner has checked `on`), timed: `res` into the ring, `applied` out of it
    void shift(const brov_result* res, double* ulog, hipStream_t st) {
        (void)timer.start(st);
        launch_delay_shift(res, applied, delay, ring, D, n, (int)B, ulog, st);
        (void)timer.stop(st);
        n++;
    }
    // the predictor on `st` ahead of a solve (the owner has checked predicts()), timed: returns where the solve reads its initial state
    const double* predict(const double* y, const PredictModel& m, hipStream_t st) {
        (void)ptimer.start(st);
        launch_delay_predict(y, m.par, m.par_stride, m.rp, m.rp_stride, ring, D, n, comp, dt_pred, xhat, (int)B, st);
        (void)ptimer.stop(st);
        predicted = true;
        return xhat;
    }

    int last_host(double* u0_applied, double* thrust_applied, const CallCtx& c) {
        if (!u0_applied && !thrust_applied) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        const char* a = (const char*)applied;
        if (u0_applied)
            BROV_HIPCHK(c.err, hipMemcpy2D(u0_applied, 4 * sizeof(double), a + offsetof(brov_result, u0), sizeof(brov_result), 4 * sizeof(double), B,
                                           hipMemcpyDeviceToHost));
        if (thrust_applied)
            BROV_HIPCHK(c.err, hipMemcpy2D(thrust_applied, 6 * sizeof(double), a + offsetof(brov_result, thrust), sizeof(brov_result),
                                           6 * sizeof(double), B, hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    // u0 [B][D][4] of the last D commanded records, oldest first: entry i is step n - D + i, zeros for a step before the first
    int queue_host(double* u0, const CallCtx& c) {
        if (!u0) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        std::vector<double> h(B * (size_t)D * 10);
        BROV_HIPCHK(c.err, hipMemcpy(h.data(), ring, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; b++)
            for (int i = 0; i < D; i++) {
                const long long step = n - D + i;
                for (int j = 0; j < 4; j++) u0[(b * D + i) * 4 + j] = step < 0 ? 0.0 : h[(b * D + (size_t)(step % D)) * 10 + j];
            }
        return BROV_OK;
    }
    // the predictor alone from `y` (null: `y_dev`, the controller's state) on `st`, to the host; moves nothing, leaves xhat and its timing alone
    int predict_host(const double* y, double* out, const double* y_dev, const PredictModel& m, const hipStream_t& st, const CallCtx& c) {
        if (!out) return c.refuse("null argument");
        for (size_t j = 0; y && j < B * 12; j++)
            if (!std::isfinite(y[j])) return c.refuse("y must be finite");
        if (int rc = ready(c)) return rc;
        const size_t nx = B * 12;
        if (y) BROV_HIPCHK(c.err, hipMemcpy(ybuf, y, nx * sizeof(double), hipMemcpyHostToDevice));
        launch_delay_predict(y ? ybuf : y_dev, m.par, m.par_stride, m.rp, m.rp_stride, ring, D, n, comp, dt_pred, ybuf + nx, (int)B, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        BROV_HIPCHK(c.err, hipMemcpy(out, ybuf + nx, nx * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int predicted_host(double* out, const CallCtx& c) {
        if (!out) return c.refuse("null argument");
        if (!predicted) return c.refuse("no solve has run the predictor since the stage was set or reset (comp > 0, brov_delay_set_host)");
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(out, xhat, B * 12 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int last_seconds(double* shift_s, double* predict_s, const CallCtx& c) {
        if (!shift_s && !predict_s) return c.refuse("null argument");
        if (shift_s && !timer.valid) return c.refuse("no plant step behind the delay stage yet");
        if (predict_s && !ptimer.valid) return c.refuse("no solve behind the predictor yet");
        if (shift_s) { if (int rc = timer.seconds(shift_s, c.err)) return rc; }
        if (predict_s) { if (int rc = ptimer.seconds(predict_s, c.err)) return rc; }
        return BROV_OK;
    }
};

}  // namespace brov
