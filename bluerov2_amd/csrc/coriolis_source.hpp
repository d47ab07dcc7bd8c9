// coriolis_source.hpp -- the host side of the plant's Coriolis stage (plant_coriolis.hip: coriolis_eval_kernel, plant_coriolis_kernel; the
// public names are brov_coriolis_* of include/bluerov2_nmpc.h): the terms in force, the stage's two coefficients, its device buffers and the
// timing of the last plant step under it.  Its owner is a brov_solver or, at batch V, a brov_fleet, whose entry points check their own handle and forward here with the
// owner's call context (CallCtx, host_common.hpp): its wait, for what may still read or write the buffers, is called once the arguments have
// passed, so a refused call changes nothing and waits for nothing.  Host code only, header only.
#pragma once
#include <cmath>

#include "host_common.hpp"
#include "nmpc_device.hpp"

namespace brov {

struct CoriolisSource : PlantStage {   // on: terms are in force (off: the plant kernels as they always were)
    CoriolisGen gen;               // what the kernels are given: gen.terms is 0 while off
    int terms_set = 0;             // the terms of the last brov_coriolis_set, which brov_coriolis_off leaves
    // [B][4] last force, [B][4] eval_host's result, [B][12] and [B][3] eval_host's arguments: from the owner's DeviceAllocs, zeroed, on first use
    double *last = nullptr, *eval = nullptr, *eval_x = nullptr, *eval_vc = nullptr;

    int terms() const { return on ? gen.terms : 0; }
    int set_off() { gen.terms = 0; return PlantStage::set_off(); }

    // behind the owner's wait: the buffers every call shares
    int ready(const CallCtx& c) {
        if (int rc = c.wait()) return rc;
        if (int rc = buffer(&last, B * 4, c)) return rc;
        gen.last = last;
        return buffer(&eval, B * 4, c);
    }
    int set(int terms, double ka, double ma, const CallCtx& c) {
        if (terms < 1 || terms > 3) return c.refuse("terms must be BROV_CORIOLIS_RIGID (1), BROV_CORIOLIS_ADDED (2) or both (3)");
        if (!std::isfinite(ka) || !std::isfinite(ma) || ka < 0.0 || ma < 0.0) return c.refuse("ka and ma must be finite and not negative");
        if (int rc = ready(c)) return rc;
        gen.terms = terms_set = terms; gen.ka = ka; gen.ma = ma;
        on = true; configured = true;
        return BROV_OK;
    }
    int get(int* terms_out, double* ka, double* ma, const CallCtx& c) const {
        if (!terms_out || !ka || !ma) return c.refuse("null argument");
        *terms_out = terms(); *ka = gen.ka; *ma = gen.ma;
        return BROV_OK;
    }
    // the force at the states x in water moving with vc (or nullptr), with the plant parameters pplant (the owner has brought them up to date on st)
    int eval_host(const double* x, const double* vc, double* out, const double* pplant, const hipStream_t& st, const CallCtx& c) {
        if (!x || !out) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        if (int rc = buffer(&eval_x, B * 12, c)) return rc;
        if (vc) { if (int rc = buffer(&eval_vc, B * 3, c)) return rc; }
        BROV_HIPCHK(c.err, hipMemcpy(eval_x, x, B * 12 * sizeof(double), hipMemcpyHostToDevice));
        if (vc) BROV_HIPCHK(c.err, hipMemcpy(eval_vc, vc, B * 3 * sizeof(double), hipMemcpyHostToDevice));
        launch_coriolis_eval(gen, pplant, (int)B, eval_x, vc ? eval_vc : nullptr, eval, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        BROV_HIPCHK(c.err, hipMemcpy(out, eval, B * 4 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int last_host(double* out, const CallCtx& c) {
        if (!out) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(out, last, B * 4 * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int last_seconds(double* seconds, const CallCtx& c) { return PlantStage::last_seconds(seconds, "no plant step under the Coriolis stage yet", c); }
    // an owner's reset (brov_fleet_reset), behind its wait: `last` to zeros; terms and coefficients stay
    int rewind(std::string& err) {
        if (last) BROV_HIPCHK(err, hipMemset(last, 0, B * 4 * sizeof(double)));
        return BROV_OK;
    }

    // one plant step under the stage on `st` (the owner has checked that it is on), timed; behind the thruster stage where th_on, g / cg: the
    // world wrench and the current in force, which may be OFF
    void step(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, double dt, int substeps, double* xlog,
              double* ulog, bool th_on, const ThrusterPar& T, const ThrusterDev& D, const WrenchGen& g, const CurrentGen& cg, long long tick,
              double* wlog, hipStream_t st) {
        (void)timer.start(st);
        launch_plant_coriolis(x0, res, pplant, prp, rp_stride, (int)B, dt, substeps, xlog, ulog, th_on, T, D, g, cg, gen, tick, wlog, st);
        (void)timer.stop(st);
    }
};

}  // namespace brov
