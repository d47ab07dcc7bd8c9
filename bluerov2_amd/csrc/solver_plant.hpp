// solver_plant.hpp -- the simulated plant of a brov_solver as one object: its true parameters, the world wrench it is under (WrenchSource),
// the delay between the controller's commands and it (DelaySource), the rotors that answer them (RotorSource), the thrust curve around those (CurveSource), the thruster stage ahead of it (ThrusterSource), the water it moves in (CurrentSource), the Coriolis forces on it (CoriolisSource), the sensor stage behind it (SensorSource), the IMU/GPS stage beside that (ImuSource), its step counter, and what the solver's entry
// points ask of them: which state the controller sees, whether the next n steps may run, whether the loop's own kernels can integrate it, and
// the one place that picks the plant kernel.  What it shares with the controller stays the solver's: non-owning pointers, given once at
// create.  The public brov_plant_* / brov_delay_* / brov_rotor_* / brov_curve_* / brov_thruster_* / brov_current_* / brov_coriolis_* / brov_sensor_* forwards stay in nmpc_api.hip.  Host code only, header only.
#pragma once
#include "coriolis_source.hpp"
#include "current_source.hpp"
#include "curve_source.hpp"
#include "delay_source.hpp"
#include "imu_source.hpp"
#include "inspect_source.hpp"
#include "rotor_source.hpp"
#include "sensor_source.hpp"
#include "thruster_source.hpp"
#include "wrench_source.hpp"

namespace brov {

void launch_copy_stage0_par(const double* par, double* pp, int B, int N1, hipStream_t st);   // copy_stage0_par_kernel (nmpc_api.hip)

// the plant update a closed loop's launch of many steps does behind every step, with its DEVICE logs
struct PlantInLaunch { double dt; int substeps; double *xlog, *ulog; };

struct SolverPlant {
    // the solver's: [B][12] true state, [B] records of the last solve, [B][N+1][16] controller parameters, and of the 6-disturbance variant
    // the controller's roll / pitch moments [B][N+1][2] (allocated by brov_enable_dist6) and the flag that call keeps up to date
    double* x0 = nullptr;
    const brov_result* res = nullptr;
    const double* par = nullptr;
    double* const* par_rp = nullptr;
    const bool* dist6 = nullptr;
    int B = 0, N = 0;
    double* pplant = nullptr;      // [B][16] true plant parameters
    double* prp_plant = nullptr;   // roll / pitch moments of the plant [B][2] (brov_plant_set_rp_disturbance_host); else the controller's stage 0
    bool pplant_set = false, prp_plant_set = false;   // explicit plant parameters / moments given (brov_plant_set_params_host, _rp_disturbance_host)
    bool pplant_stale = true;      // controller parameters changed since the plant's copy of them was taken
    WrenchSource wr;               // world-frame wrench (brov_plant_wrench_*), its buffers allocated on first use; it stores the step counter
    ThrusterSource th;             // thruster stage (brov_thruster_*): limits, faults and propulsion matrix, its buffers allocated on first use
    CurrentSource cu;              // ocean current (brov_current_*): a world-frame water velocity, its buffers allocated on first use
    CoriolisSource co;             // Coriolis stage (brov_coriolis_*): the forces the OCP model drops, its buffers allocated on first use
    SensorSource sn;               // sensor stage (brov_sensor_*): the measured state, its buffers allocated on first use
    ImuSource im;                  // IMU/GPS stage (brov_imu_*): what the error-state filter reads, from the true state, its buffers allocated on first use
    InspectSource in;              // range stage and inspection controller (brov_range_*, brov_inspect_*): writes the records in the solver's place, its buffers allocated on first use
    DelaySource dl;                // delay stage (brov_delay_*): the queue of commanded records and the predictor, its buffers allocated on first use
    RotorSource ro;                // rotor stage (brov_rotor_*): first-order dynamics of the thrusters behind the delay, its buffers allocated on first use
    CurveSource cv;                // thrust-curve stage (brov_curve_*): command map and ESC steps ahead of the rotors, conversion curve and efficiency behind them, its buffers allocated on first use

    void init(int B_, int N_, double* x0_, const brov_result* res_, const double* par_, double* const* par_rp_, const bool* dist6_) {
        B = B_; N = N_; x0 = x0_; res = res_; par = par_; par_rp = par_rp_; dist6 = dist6_;
        wr.B = th.B = cu.B = co.B = sn.B = im.B = in.B = dl.B = ro.B = cv.B = (size_t)B_;
    }
    void destroy() { wr.destroy(); th.destroy(); cu.destroy(); co.destroy(); sn.destroy(); im.destroy(); in.destroy(); dl.destroy(); ro.destroy(); cv.destroy(); }

    long long tick() const { return wr.tick; }   // plant steps so far (brov_plant_wrench_seek sets it): the wrench's tick, the sensor's index
    // may the next `n` steps run?  The wrench's generator, then the current's draws, then the sensor's index
    int steps_ok(long long n, const CallCtx& c) const {
        if (int rc = wr.steps_ok(n, c)) return rc;
        if (int rc = cu.steps_ok(wr.tick, n, c)) return rc;
        if (int rc = sn.steps_ok(wr.tick, n, c)) return rc;
        return im.steps_ok(wr.tick, n, c);
    }
    // may a step of length `dt` run?  The rotor stage's coefficients hold for one step length alone, and so do the IMU stage's differencing and the inspection controller's period
    int dt_ok(double dt, const CallCtx& c) const {
        if (int rc = ro.dt_ok(dt, c)) return rc;
        if (int rc = im.dt_ok(dt, c)) return rc;
        return in.dt_ok(dt, c);
    }
    // no stage in force: the *_ticks kernels, which integrate the plant themselves and know none of them, can run the loop in one launch
    bool plain() const { return wr.off() && !th.on && cu.off() && !co.on && !sn.on && !im.on && !dl.on && !ro.on && !cv.on; }

    // what the controller knows of the state: the measured state while the sensor stage is on, else the true one
    const double* controller_state() const { return sn.on ? sn.ymeas : x0; }
    // the model the delay stage's predictor integrates: the controller's own stage-0 parameters and, 6-disturbance variant, its moments
    PredictModel predict_model(const double* par_in = nullptr) const {
        return {par_in ? par_in : par, (N + 1) * 16, *dist6 ? *par_rp : nullptr, (N + 1) * 2};
    }
    // the delay stage predicts (the owner has asked dl.predicts()): x^ from what the controller knows of the state, on `st`; where the solve reads it
    const double* predict(const double* par_in, hipStream_t st) { return dl.predict(controller_state(), predict_model(par_in), st); }
    // ... of a brov_tick_host that brought its own x0, the caller's measurement: where its kernel reads it in place, else x0, where it was copied
    const double* tick_state(bool x0_passed, const double* in_place) const { return sn.on && x0_passed && !in_place ? x0 : in_place; }
    // a caller rewrites the true state: the measured state follows it with a forced refresh at the counter's index, which must be one
    // (the IMU stage restarts likewise)
    int rewrite_ok(const CallCtx& c) const {
        if (sn.on) { if (int rc = SensorSource::index_ok(wr.tick, c)) return rc; }
        return im.on ? ImuSource::index_ok(wr.tick, c) : BROV_OK;
    }
    bool rewritten(hipStream_t st) {
        if (sn.on) sn.measure(x0, wr.tick, true, st);
        if (im.on) im.measure(x0, wr.tick, true, st);
        return sn.on || im.on;
    }

    // Without explicit plant parameters the plant is the controller's own model: stage-0 parameters, re-read whenever the controller's
    // parameters may have changed (setters, brov_params_device() hand-outs, the EKF's write-back).
    void params_changed() { pplant_stale = true; }
    void ensure_params(hipStream_t st) {
        if (!pplant_set && pplant_stale) { launch_copy_stage0_par(par, pplant, B, N + 1, st); pplant_stale = false; }
    }
    // roll / pitch disturbance moments the plant integrates (6-disturbance variant): its own, else the controller's stage 0, else none
    const double* rp() const { return prp_plant_set ? prp_plant : (*dist6 && !pplant_set ? *par_rp : nullptr); }
    int rp_stride() const { return prp_plant_set ? 2 : (N + 1) * 2; }

    // one plant step at the counter's tick on `st`, with optional DEVICE logs of this tick: the one place that picks the plant kernel (thruster
    // stage off and both modes OFF: as it always was; a current in force: its kernel, which knows the other two; the Coriolis stage on: its
    // kernel, which knows the other three).  Sensor stage on: a regular refresh behind it at the counter's new value (the caller has asked steps_ok)
    void step(double dt, int substeps, double* xlog, double* ulog, double* wlog, hipStream_t st) {
        // delay stage on: its step ahead of the plant kernel, which then reads the applied records; the `u` log is the stage's, the commanded input
        const brov_result* rec = res;
        if (dl.on) { dl.shift(res, ulog, st); rec = dl.applied; ulog = nullptr; }
        // rotor stage on: behind the delay, ahead of the thruster stage; it lags the record that arrives and logs the commanded input likewise
        // thrust-curve stage on: its COMMAND part ahead of the rotors and its THRUST part behind them; rotor stage off: both in one launch
        if (cv.on && !ro.on) { cv.both(rec, dt, ulog, st); rec = cv.applied; ulog = nullptr; }
        if (cv.on && ro.on) { cv.command(rec, ulog, st); rec = cv.applied_cmd; ulog = nullptr; }
        if (ro.on) { ro.shift(rec, ulog, st); rec = ro.applied; ulog = nullptr; }
        if (cv.on && ro.on) { cv.thrust(rec, dt, st); rec = cv.applied; }
        if (co.on) {
            if (th.on) (void)th.timer.start(st);     // the thruster stage's timing and step count, as its own step() keeps them ...
            if (!cu.off()) (void)cu.timer.start(st);   // ... and the current's, as its own
            co.step(x0, rec, pplant, rp(), rp_stride(), dt, substeps, xlog, ulog, th.on, th.par, th.dev, wr.gen, cu.gen, wr.tick, wlog, st);
            if (!cu.off()) (void)cu.timer.stop(st);
            if (th.on) { (void)th.timer.stop(st); th.steps++; }
        } else if (!cu.off()) {
            if (th.on) (void)th.timer.start(st);   // the thruster stage's timing and step count, as its own step() keeps them
            cu.step(x0, rec, pplant, rp(), rp_stride(), dt, substeps, xlog, ulog, th.on, th.par, th.dev, wr.gen, wr.tick, wlog, st);
            if (th.on) { (void)th.timer.stop(st); th.steps++; }
        } else if (th.on) th.step(x0, rec, pplant, rp(), rp_stride(), dt, substeps, xlog, ulog, wr.gen, wr.tick, wlog, st);
        else if (wr.off()) launch_plant(x0, rec, pplant, rp(), rp_stride(), B, dt, substeps, xlog, ulog, st);
        else launch_plant_wrench(x0, rec, pplant, rp(), rp_stride(), B, dt, substeps, xlog, ulog, wr.gen, wr.tick, wlog, st);
        wr.tick++;
        if (sn.on) sn.measure(x0, wr.tick, false, st);
        if (im.on) im.measure(x0, wr.tick, false, st);
    }
    // the plain plant (the owner has asked) into a launch of P.ticks steps: what the kernel integrates it with; the counter moves on by those steps
    void into_ticks(DevParams& P, const PlantInLaunch& in) {
        P.plant_pp = pplant; P.plant_rp = rp(); P.plant_rp_stride = rp_stride(); P.plant_substeps = in.substeps; P.plant_dt = in.dt;
        P.x0_rw = x0; P.plant_xlog = in.xlog; P.plant_ulog = in.ulog;
        wr.tick += P.ticks;
    }
};

}  // namespace brov
