// curve_source.hpp -- the host side of the plant's thrust-curve stage (curve_kernel.hip: curve_shift_kernel<PART>, curve_eval_kernel; the public
// names are brov_curve_* of include/bluerov2_nmpc_curve.h): the configuration in force, the two tables with their slopes, which are computed
// HERE, in doubles, and uploaded as the images the kernels stage in LDS, the efficiencies, the applied records of both parts and the books on
// the device, the stage's own step count and the timing of the last launch of either part.  Its owner is a brov_solver, whose entry points
// check their own handle and forward here with the owner's call context (CallCtx, host_common.hpp): its wait is called once the arguments
// have passed, so a refused call changes nothing and waits for nothing.  Shares PlantStage with the other stages.  Host code only, header only.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

struct CurveSource : PlantStage {   // on: the plant steps read the applied records (off: what they read without the stage)
    struct Table {                  // the host's copy of an uploaded table
        std::vector<double> x, y, slope, amps, amps_slope;
        bool has_amps = false;
        int K() const { return (int)x.size(); }
    };
    CurvePar par;                   // modes, constants and the tables' sizes in force
    Table tab[2];                   // BROV_CURVE_WHICH_CURVE, _PRE
    double* img[2] = {nullptr, nullptr};   // the tables' device images (curve_image_doubles), room for 256 knots each
    double* eff = nullptr;          // [B][6]
    CurveBooks bk = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    brov_result* applied_cmd = nullptr;   // [B] what the COMMAND part handed to the rotor stage
    brov_result* applied = nullptr;       // [B] what the last plant step was given
    double* eval = nullptr;         // [3][B][6] of eval_host: in, out, amps
    KernelTimer timer_cmd;          // around the last COMMAND launch (PlantStage::timer: THRUST or BOTH)
    bool last_both = false;         // the last step was one BOTH launch
    bool observer_applied = false;  // brov_ekf_update_from_solver reads the applied records
    long long steps = 0;            // steps of the stage since it was set or reset

    static void default_params(brov_curve_params* p) {
        if (!p) return;
        *p = brov_curve_params{};
        p->kind = BROV_CURVE_LINEAR; p->pre = BROV_CURVE_PRE_NONE;
        p->k = p->kl = p->kr = 1.0;
        p->pre_poly[3] = 1.0;
    }
    static void to_par(const brov_curve_params& p, CurvePar* q) {
        q->kind = p.kind; q->pre = p.pre;
        q->quantum = p.quantum; q->inv_quantum = p.quantum > 0.0 ? 1.0 / p.quantum : 0.0;
        q->k = p.k; q->kl = p.kl; q->kr = p.kr; q->dl = p.dl; q->dr = p.dr;
        for (int i = 0; i < 5; i++) q->pre_poly[i] = p.pre_poly[i];
    }
    void destroy() { timer_cmd.destroy(); PlantStage::destroy(); }

    // the buffers on first use; the default configuration is a copy: LINEAR, PRE_NONE, no quantum, every efficiency 1, no table
    int ensure(const CallCtx& c) {
        const size_t n = B * 6;
        for (int w = 0; w < 2; w++)
            if (int rc = buffer(&img[w], (size_t)curve_image_doubles(BROV_CURVE_MAX_KNOTS, w == BROV_CURVE_WHICH_CURVE), c)) return rc;
        const bool fresh = !eff;
        if (int rc = buffer(&eff, n, c)) return rc;
        if (int rc = buffer(&bk.wanted, n, c)) return rc;
        if (int rc = buffer(&bk.last_command, n, c)) return rc;
        if (int rc = buffer(&bk.last_thrust, n, c)) return rc;
        if (int rc = buffer(&bk.err_sq, B, c)) return rc;
        if (int rc = buffer(&bk.charge, B, c)) return rc;
        if (int rc = buffer(&bk.dead_ticks, n, c)) return rc;
        if (int rc = buffer(&applied_cmd, B, c)) return rc;
        if (int rc = buffer(&applied, B, c)) return rc;
        if (int rc = buffer(&eval, 3 * n, c)) return rc;
        if (!timer_cmd.ev[0]) BROV_HIPCHK(c.err, timer_cmd.create());
        if (fresh) {
            const std::vector<double> one(n, 1.0);
            BROV_HIPCHK(c.err, hipMemcpy(eff, one.data(), n * sizeof(double), hipMemcpyHostToDevice));
        }
        if (!configured) {
            brov_curve_params p;
            default_params(&p);
            const int Kc = par.Kc, Kp = par.Kp, am = par.amps;
            to_par(p, &par);
            par.Kc = Kc; par.Kp = Kp; par.amps = am; par.reserved_ = 0;
            configured = true;
        }
        return BROV_OK;
    }
    CurveSource() { par = CurvePar{}; }
    int ready(const CallCtx& c) { const int rc = c.wait(); return rc ? rc : ensure(c); }
    int clear_stats(std::string& err) {
        BROV_HIPCHK(err, hipMemset(bk.err_sq, 0, B * sizeof(double)));
        BROV_HIPCHK(err, hipMemset(bk.charge, 0, B * sizeof(double)));
        BROV_HIPCHK(err, hipMemset(bk.dead_ticks, 0, B * 6 * sizeof(int32_t)));
        steps = 0;
        return BROV_OK;
    }
    // the books, the applied records and the step count to zero; the caller has waited
    int clear(std::string& err) {
        BROV_HIPCHK(err, hipMemset(bk.wanted, 0, B * 6 * sizeof(double)));
        BROV_HIPCHK(err, hipMemset(bk.last_command, 0, B * 6 * sizeof(double)));
        BROV_HIPCHK(err, hipMemset(bk.last_thrust, 0, B * 6 * sizeof(double)));
        BROV_HIPCHK(err, hipMemset(applied_cmd, 0, B * sizeof(brov_result)));
        BROV_HIPCHK(err, hipMemset(applied, 0, B * sizeof(brov_result)));
        return clear_stats(err);
    }
    int reset(const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        return clear(c.err);
    }
    int reset_stats(const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        return clear_stats(c.err);
    }

    int set_table_host(int32_t which, const double* x, const double* y, const double* amps, int32_t K, const CallCtx& c) {
        if (which != BROV_CURVE_WHICH_CURVE && which != BROV_CURVE_WHICH_PRE) return c.refuse("unknown table (BROV_CURVE_WHICH_*)");
        if (K < 2 || K > BROV_CURVE_MAX_KNOTS) return c.refuse("K must be in [2, 256]");
        if (!x || !y) return c.refuse("null argument");
        if (amps && which != BROV_CURVE_WHICH_CURVE) return c.refuse("the pre table has no amps column");
        Table t;
        t.has_amps = amps != nullptr;
        t.x.assign(x, x + K); t.y.assign(y, y + K);
        t.amps.assign(K, 0.0); t.slope.assign(K, 0.0); t.amps_slope.assign(K, 0.0);
        for (int j = 0; j < K; j++) {
            if (amps) t.amps[j] = amps[j];
            if (!std::isfinite(x[j]) || !std::isfinite(y[j]) || !std::isfinite(t.amps[j])) return c.refuse("a table value is not finite");
            if (j && !(x[j] > x[j - 1])) return c.refuse("the knots are not strictly increasing");
        }
        for (int j = 0; j + 1 < K; j++) {
            const double dx = x[j + 1] - x[j];
            t.slope[j] = (y[j + 1] - y[j]) / dx;
            t.amps_slope[j] = (t.amps[j + 1] - t.amps[j]) / dx;
            if (!std::isfinite(t.slope[j]) || !std::isfinite(t.amps_slope[j])) return c.refuse("a table value is not finite: a slope overflows");
        }
        const int Ke = (K + 1) & ~1;
        std::vector<double> image((size_t)curve_image_doubles(K, t.has_amps), 0.0);
        for (int j = 0; j < K; j++) {
            image[j] = t.x[j];
            image[Ke + 2 * j] = t.y[j]; image[Ke + 2 * j + 1] = t.slope[j];
            if (t.has_amps) { image[Ke + 2 * K + 2 * j] = t.amps[j]; image[Ke + 2 * K + 2 * j + 1] = t.amps_slope[j]; }
        }
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(img[which], image.data(), image.size() * sizeof(double), hipMemcpyHostToDevice));
        if (which == BROV_CURVE_WHICH_CURVE) { par.Kc = K; par.amps = t.has_amps ? 1 : 0; } else par.Kp = K;
        tab[which] = std::move(t);
        return BROV_OK;
    }
    int get_table_host(int32_t which, double* x, double* y, double* slope, double* amps, double* amps_slope, int32_t* K, const CallCtx& c) const {
        if (which != BROV_CURVE_WHICH_CURVE && which != BROV_CURVE_WHICH_PRE) return c.refuse("unknown table (BROV_CURVE_WHICH_*)");
        if (!K) return c.refuse("null argument");
        const Table& t = tab[which];
        *K = t.K();
        for (int j = 0; j < t.K(); j++) {
            if (x) x[j] = t.x[j];
            if (y) y[j] = t.y[j];
            if (slope) slope[j] = t.slope[j];
            if (amps) amps[j] = t.amps[j];
            if (amps_slope) amps_slope[j] = t.amps_slope[j];
        }
        return BROV_OK;
    }

    int set_host(const brov_curve_params* p, const double* eff_, const CallCtx& c) {
        if (!p) return c.refuse("null argument");
        if (p->kind < BROV_CURVE_LINEAR || p->kind > BROV_CURVE_TABLE) return c.refuse("unknown kind (BROV_CURVE_LINEAR ... BROV_CURVE_TABLE)");
        if (p->pre < BROV_CURVE_PRE_NONE || p->pre > BROV_CURVE_PRE_TABLE) return c.refuse("unknown pre (BROV_CURVE_PRE_NONE ... BROV_CURVE_PRE_TABLE)");
        if (!std::isfinite(p->quantum) || p->quantum < 0.0) return c.refuse("quantum must be finite and >= 0");
        if (!std::isfinite(p->k) || !std::isfinite(p->kl) || !std::isfinite(p->kr) || !std::isfinite(p->dl) || !std::isfinite(p->dr))
            return c.refuse("k, kl, kr, dl and dr must be finite");
        if (p->dl > p->dr) return c.refuse("dl > dr: the dead zone is empty");
        for (int i = 0; i < 5; i++)
            if (!std::isfinite(p->pre_poly[i])) return c.refuse("a polynomial coefficient is not finite");
        if (p->quantum > 0.0 && !std::isfinite(1.0 / p->quantum)) return c.refuse("quantum must be finite and >= 0: its reciprocal overflows");
        for (size_t j = 0; eff_ && j < B * 6; j++)
            if (!std::isfinite(eff_[j])) return c.refuse("eff must be finite");
        if (p->kind == BROV_CURVE_TABLE && par.Kc < 2) return c.refuse("BROV_CURVE_TABLE with no curve table set (brov_curve_set_table_host)");
        if (p->pre == BROV_CURVE_PRE_TABLE && par.Kp < 2) return c.refuse("BROV_CURVE_PRE_TABLE with no pre table set (brov_curve_set_table_host)");
        if (int rc = ready(c)) return rc;
        const std::vector<double> one(eff_ ? 0 : B * 6, 1.0);
        BROV_HIPCHK(c.err, hipMemcpy(eff, eff_ ? eff_ : one.data(), B * 6 * sizeof(double), hipMemcpyHostToDevice));
        to_par(*p, &par);
        observer_applied = p->observer_applied != 0;
        if (int rc = clear(c.err)) return rc;
        on = true;
        return BROV_OK;
    }

    // the parts of one plant step on `st` (the owner has checked `on`), timed.  Rotor stage off: both(); on: command() ahead of its shift and
    // thrust() behind it
    void both(const brov_result* rec, double dt, double* ulog, hipStream_t st) {
        (void)timer.start(st);
        launch_curve_shift(CURVE_BOTH, rec, applied, par, eff, img[0], img[1], bk, dt, (int)B, ulog, st);
        (void)timer.stop(st);
        last_both = true;
        steps++;
    }
    void command(const brov_result* rec, double* ulog, hipStream_t st) {
        (void)timer_cmd.start(st);
        launch_curve_shift(CURVE_COMMAND, rec, applied_cmd, par, eff, img[0], img[1], bk, 0.0, (int)B, ulog, st);
        (void)timer_cmd.stop(st);
    }
    void thrust(const brov_result* rec, double dt, hipStream_t st) {
        (void)timer.start(st);
        launch_curve_shift(CURVE_THRUST, rec, applied, par, eff, img[0], img[1], bk, dt, (int)B, nullptr, st);
        (void)timer.stop(st);
        last_both = false;
        steps++;
    }

    int eval_host(int32_t part, const double* in, double* out, double* amps_out, const hipStream_t& st, const CallCtx& c) {
        if (part != CURVE_COMMAND && part != CURVE_THRUST && part != CURVE_BOTH) return c.refuse("unknown part (BROV_CURVE_PART_*)");
        if (!in || !out) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        const size_t n = B * 6;
        BROV_HIPCHK(c.err, hipMemcpy(eval, in, n * sizeof(double), hipMemcpyHostToDevice));
        launch_curve_eval(part, par, eff, img[0], img[1], eval, eval + n, eval + 2 * n, (int)B, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        BROV_HIPCHK(c.err, hipMemcpy(out, eval + n, n * sizeof(double), hipMemcpyDeviceToHost));
        if (amps_out) BROV_HIPCHK(c.err, hipMemcpy(amps_out, eval + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int last_host(double* u0_applied, double* wanted, double* command_, double* thrust_, const CallCtx& c) {
        if (!u0_applied && !wanted && !command_ && !thrust_) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        if (u0_applied)
            BROV_HIPCHK(c.err, hipMemcpy2D(u0_applied, 4 * sizeof(double), (const char*)applied + offsetof(brov_result, u0), sizeof(brov_result),
                                           4 * sizeof(double), B, hipMemcpyDeviceToHost));
        if (wanted) BROV_HIPCHK(c.err, hipMemcpy(wanted, bk.wanted, B * 6 * sizeof(double), hipMemcpyDeviceToHost));
        if (command_) BROV_HIPCHK(c.err, hipMemcpy(command_, bk.last_command, B * 6 * sizeof(double), hipMemcpyDeviceToHost));
        if (thrust_) BROV_HIPCHK(c.err, hipMemcpy(thrust_, bk.last_thrust, B * 6 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_stats_host(double* err_sq, int32_t* dead_ticks, double* charge, int64_t* steps_out, const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        if (err_sq) BROV_HIPCHK(c.err, hipMemcpy(err_sq, bk.err_sq, B * sizeof(double), hipMemcpyDeviceToHost));
        if (dead_ticks) BROV_HIPCHK(c.err, hipMemcpy(dead_ticks, bk.dead_ticks, B * 6 * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (charge) BROV_HIPCHK(c.err, hipMemcpy(charge, bk.charge, B * sizeof(double), hipMemcpyDeviceToHost));
        if (steps_out) *steps_out = (int64_t)steps;
        return BROV_OK;
    }
    int last_seconds(double* command_s, double* thrust_s, const CallCtx& c) {
        if (!command_s && !thrust_s) return c.refuse("null argument");
        KernelTimer& tc = last_both ? timer : timer_cmd;
        if ((thrust_s && !timer.valid) || (command_s && !tc.valid)) return c.refuse("no plant step behind the thrust-curve stage yet");
        if (command_s) { if (int rc = tc.seconds(command_s, c.err)) return rc; }
        if (thrust_s) { if (int rc = timer.seconds(thrust_s, c.err)) return rc; }
        return BROV_OK;
    }
};

}  // namespace brov
