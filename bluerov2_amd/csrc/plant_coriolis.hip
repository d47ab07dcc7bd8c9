// plant_coriolis.hip -- the device plant with the Coriolis and centripetal forces the OCP model drops (brov_coriolis_* of
// include/bluerov2_nmpc.h): the vehicle the reference's observer is written for (BLUEROV2_DOB::f(), bluerov2_dob.cpp:651-677: the rigid-body
// products on x, y, z; dynamics_C(), :894-906: C_RB + C_A).  The forces depend on the state, so neither the world wrench nor the body-frame
// parameters p[0..3] can pose them: they are evaluated afresh at every RK stage (model_f<WorldWrenchCurrentCoriolis>, bluerov2_model.hpp;
// coriolis_force, plant_stages.hpp).
// coriolis_eval_kernel: the force alone, for given states and optional world-frame water velocities.  plant_coriolis_kernel<TH, WR>: the plant
// step of plant_current_kernel with the stage on top: gather -> thruster stage and its accounting (TH) -> world wrench at the tick (WR) -> current
// at the tick -> the stage's force at the start state into `last` -> plant_erk4 under the fourth tag -> store / logs -> Gauss-Markov advance.
// The thruster stage and the world wrench are template parameters, as in plant_current.hip; the current is RUN-TIME here: a mode that is off
// gives zeros, and a zero current changes no bit of a finite state (v - 0 is exact), so four instantiations stand, not eight.  (With the
// wrench at run time as well the instantiation without one carried 2424 instructions against 1982 and ran 2 us longer at B = 262 144.)  One
// lane per instance, FP64, no LDS, no scratch, no atomics.
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"
#include "plant_stages.hpp"   // wrench_at, thruster_stage, thruster_account, coriolis_force, water_velocity
#include "current_gen.hpp"    // current_at, current_advance

namespace brov {

// c[b] = the stage's force [X Y Z N] at the state x[b], in water that moves with vc[b] (vc = nullptr: still water, the velocity through the
// water IS x[6..9)), with the added masses of the plant parameters pplant[b][4..7)
__global__ __launch_bounds__(128) void coriolis_eval_kernel(CoriolisGen co, const double* __restrict__ pplant, int B, const double* __restrict__ xs,
                                                            const double* __restrict__ vcs, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[NX], c[4], nr[3];
#pragma unroll
    for (int j = 0; j < NX; j++) x[j] = xs[(size_t)b * NX + j];
    const CoriolisStage cs = {co.terms, pplant[(size_t)b * NP + 4], pplant[(size_t)b * NP + 5], pplant[(size_t)b * NP + 6], co.ka, co.ma};
    if (vcs) {
        const double vc[3] = {vcs[(size_t)b * 3], vcs[(size_t)b * 3 + 1], vcs[(size_t)b * 3 + 2]};
        water_velocity(x, vc, nr);
    } else {
        nr[0] = x[6]; nr[1] = x[7]; nr[2] = x[8];
    }
    const double nu[6] = {x[6], x[7], x[8], x[9], x[10], x[11]};
    coriolis_force(cs, nu, nr, c);
    store_row(out + (size_t)b * 4, c);
}

// TH: behind the thruster stage, as plant_current_kernel<true, .> writes it; else the wrench of plant_inputs.  WR: the generator `gen` at
// `tick` on top, logged into wlog; else a zero world wrench, which folds away.  cg: the current in force, which may be OFF (then cg.last is
// not written: it exists only once a current was set).
template <bool TH, bool WR>
__global__ __launch_bounds__(128) void plant_coriolis_kernel(double* __restrict__ x0, const brov_result* __restrict__ res,
                                                             const double* __restrict__ pplant, const double* __restrict__ prp, int rp_stride, int B,
                                                             double dt, int substeps, double* __restrict__ xlog, double* __restrict__ ulog,
                                                             ThrusterPar T, ThrusterDev D, WrenchGen gen, CurrentGen cg, CoriolisGen co, long long tick,
                                                             double* __restrict__ wlog) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[NX], u[NU], vc[3], wv[6];
    ModelPar m;
    Wrench w;
    plant_inputs(x0 + (size_t)b * NX, res[b].u0, pplant + (size_t)b * NP, prp, (size_t)b * rp_stride, x, u, m, w);
    if constexpr (TH) {
        double t[6], a[6], g[6];
#pragma unroll
        for (int i = 0; i < 6; i++) t[i] = res[b].thrust[i];
        thruster_stage(T, D, b, tick, t, a, g);
        thruster_account(T, D, b, t, a);
        w.k0 = g[0]; w.k1 = g[1]; w.k2 = g[2]; w.k3 = g[3]; w.k4 = g[4]; w.k5 = g[5];
        if (prp) { w.k3 += prp[(size_t)b * rp_stride]; w.k4 += prp[(size_t)b * rp_stride + 1]; }   // 6-disturbance variant
    }
    WorldWrenchCurrentCoriolis wc;
    wc.wc.ww = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (WR) {
        wrench_at(gen, b, tick, wv);
        wc.wc.ww = {wv[0], wv[1], wv[2], wv[3], wv[4], wv[5]};   // held over the tick
        log_row(wlog, b, wv);
    }
    current_at(cg, b, tick, vc);   // OFF: zeros
    wc.wc.vx = vc[0]; wc.wc.vy = vc[1]; wc.wc.vz = vc[2];   // held over the tick
    if (cg.mode != BROV_CURRENT_OFF) store_row(cg.last + (size_t)b * 3, vc);
    wc.cs = {co.terms, pplant[(size_t)b * NP + 4], pplant[(size_t)b * NP + 5], pplant[(size_t)b * NP + 6], co.ka, co.ma};
    {   // the stage's force at the start state, as coriolis_eval_kernel gives it
        double c[4], nr[3] = {x[6], x[7], x[8]};
        if (cg.mode != BROV_CURRENT_OFF) water_velocity(x, vc, nr);
        const double nu[6] = {x[6], x[7], x[8], x[9], x[10], x[11]};
        coriolis_force(wc.cs, nu, nr, c);
        store_row(co.last + (size_t)b * 4, c);
    }
    log_row(ulog, b, u);
    plant_erk4(x, w, m, wc, dt, substeps);
    store_row(x0 + (size_t)b * NX, x);
    log_row(xlog, b, x);
    if (cg.mode == BROV_CURRENT_GAUSS_MARKOV) current_advance(cg, b, tick, vc);
}

void launch_plant_coriolis(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, int B, double dt, int substeps,
                           double* xlog, double* ulog, bool th_on, const ThrusterPar& T, const ThrusterDev& D, const WrenchGen& g, const CurrentGen& cg,
                           const CoriolisGen& co, long long tick, double* wlog, hipStream_t st) {
    const dim3 grid((B + 127) / 128), block(128);
    const bool wr_on = g.mode != BROV_WRENCH_OFF;
#define BROV_LAUNCH_CORIOLIS(TH, WR) \
    hipLaunchKernelGGL((plant_coriolis_kernel<TH, WR>), grid, block, 0, st, x0, res, pplant, prp, rp_stride, B, dt, substeps, xlog, ulog, T, D, g, cg, co, tick, wlog)
    if (th_on && wr_on) BROV_LAUNCH_CORIOLIS(true, true);
    else if (th_on) BROV_LAUNCH_CORIOLIS(true, false);
    else if (wr_on) BROV_LAUNCH_CORIOLIS(false, true);
    else BROV_LAUNCH_CORIOLIS(false, false);
#undef BROV_LAUNCH_CORIOLIS
}
void launch_coriolis_eval(const CoriolisGen& co, const double* pplant, int B, const double* x, const double* vc, double* out, hipStream_t st) {
    hipLaunchKernelGGL(coriolis_eval_kernel, dim3((B + 127) / 128), dim3(128), 0, st, co, pplant, B, x, vc, out);
}

}  // namespace brov
