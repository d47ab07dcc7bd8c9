// plant_current.hip -- the device plant in moving water (brov_current_* of include/bluerov2_nmpc.h): the constant_current block of the
// reference's simulated world (bluerov2_environ/worlds/ocean_waves.world, underwater_current_plugin), which neither the world wrench nor the
// body-frame parameters p[0..3] can pose: the drag a current causes depends on the vehicle's own velocity and attitude.
//   constant       [B][3] world-frame water velocity
//   table          [rows][3], one row per plant tick, the last row repeated past the end, times an optional per-instance gain
//   Gauss-Markov   the plugin's first-order process per world axis, device state c[B][3], advanced behind every plant step
// current_eval_kernel: the generator alone (constant / table).  plant_current_kernel<TH, WR>: the plant step of plant_thruster_kernel /
// plant_wrench_kernel with the current on top: gather -> thruster stage and its accounting (TH) -> world wrench at the tick (WR) -> current at
// the tick -> plant_erk4 under model_f<WorldWrenchCurrent> -> store / logs -> Gauss-Markov advance.  One lane per instance, FP64, no scratch,
// no atomics.  The generator's arithmetic is written with the singly rounded operations of rounded_ops.hpp: the kernels and the numpy
// restatement of tests/current_restatement.py agree bit for bit.
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"
#include "plant_stages.hpp"   // wrench_at, thruster_stage, thruster_account
#include "current_gen.hpp"    // current_at, current_advance

namespace brov {

__global__ __launch_bounds__(128) void current_eval_kernel(CurrentGen g, int B, long long tick, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double v[3];
    current_at(g, b, tick, v);
    store_row(out + (size_t)b * 3, v);
}

// TH: behind the thruster stage, written as plant_thruster_kernel does it (the wrench of the step is the stage's g, the roll / pitch moments of
// the 6-disturbance variant ADDED to its k3, k4), with the same statistics; else the wrench of plant_inputs.  WR: the generator `gen` at
// `tick` on top, logged into wlog as plant_wrench_kernel does; else a zero world wrench, which folds away.  The `u` log stays the commanded input.
template <bool TH, bool WR>
__global__ __launch_bounds__(128) void plant_current_kernel(double* __restrict__ x0, const brov_result* __restrict__ res,
                                                            const double* __restrict__ pplant, const double* __restrict__ prp, int rp_stride, int B,
                                                            double dt, int substeps, double* __restrict__ xlog, double* __restrict__ ulog,
                                                            ThrusterPar T, ThrusterDev D, WrenchGen gen, CurrentGen cg, long long tick,
                                                            double* __restrict__ wlog) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[NX], u[NU], vc[3];
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
    WorldWrenchCurrent wc = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};
    if constexpr (WR) {
        double wv[6];
        wrench_at(gen, b, tick, wv);
        wc.ww = {wv[0], wv[1], wv[2], wv[3], wv[4], wv[5]};   // held over the tick
        log_row(wlog, b, wv);
    }
    current_at(cg, b, tick, vc);
    wc.vx = vc[0]; wc.vy = vc[1]; wc.vz = vc[2];   // held over the tick
    store_row(cg.last + (size_t)b * 3, vc);
    plant_erk4(x, w, m, wc, dt, substeps);
    store_row(x0 + (size_t)b * NX, x);
    log_row(xlog, b, x);
    log_row(ulog, b, u);
    if (cg.mode == BROV_CURRENT_GAUSS_MARKOV) current_advance(cg, b, tick, vc);
}

void launch_plant_current(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, int B, double dt, int substeps,
                          double* xlog, double* ulog, bool th_on, const ThrusterPar& T, const ThrusterDev& D, const WrenchGen& g, const CurrentGen& cg,
                          long long tick, double* wlog, hipStream_t st) {
    const dim3 grid((B + 127) / 128), block(128);
    const bool wr_on = g.mode != BROV_WRENCH_OFF;
#define BROV_LAUNCH_CURRENT(TH, WR) \
    hipLaunchKernelGGL((plant_current_kernel<TH, WR>), grid, block, 0, st, x0, res, pplant, prp, rp_stride, B, dt, substeps, xlog, ulog, T, D, g, cg, tick, wlog)
    if (th_on && wr_on) BROV_LAUNCH_CURRENT(true, true);
    else if (th_on) BROV_LAUNCH_CURRENT(true, false);
    else if (wr_on) BROV_LAUNCH_CURRENT(false, true);
    else BROV_LAUNCH_CURRENT(false, false);
#undef BROV_LAUNCH_CURRENT
}
void launch_current_eval(const CurrentGen& cg, int B, long long tick, double* out, hipStream_t st) {
    hipLaunchKernelGGL(current_eval_kernel, dim3((B + 127) / 128), dim3(128), 0, st, cg, B, tick, out);
}

}  // namespace brov
