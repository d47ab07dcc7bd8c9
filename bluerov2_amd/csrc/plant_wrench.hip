// plant_wrench.hip -- the device plant under a time-varying WORLD-frame wrench: the disturbance scenarios of the reference's
// applyBodyWrench() (bluerov2_dobmpc/src/bluerov2_dob.cpp:754-892; bluerov2_ampc.cpp:1050-1150 is the same code with a
// slower phase rate), which the constant body-frame parameters p[0..3] of the plant cannot pose:
//   constant   (10, 10, 10, 0) N / Nm in the world frame (:813-816)
//   periodic   sin(t) times amplitudes redrawn every half period (:776-795), the yaw torque from the Y amplitude (:787)
//   table      recorded force / torque rows, one per tick (:869-873)
// The wrench of instance b at tick k is a pure function of (generator data, b, k): no generator state lives on the device, any tick can be
// evaluated again (brov_plant_wrench_eval_host).  The arithmetic of the generator is written with explicitly rounded operations under
// `fp contract(off)` (hipcc otherwise contracts a product and a sum into an FMA, also across inlined calls): the evaluation kernel, the plant kernel and the numpy restatement of tests/wrench_restatement.py then agree bit for bit
// except through sin().  (The generator, wrench_at, and the thruster stage's two functions live in plant_stages.hpp, which plant_current.hip shares.)
// plant_kernel / plant_wrench_kernel: the plant update of the closed loops without / with such a wrench: one lane per instance, FP64, no
// scratch.  plant_kernel is the device's one plant step (bluerov2_model.hpp: plant_inputs, plant_erk4, store_row / log_row);
// plant_wrench_kernel restates it (see there) with the wrench projected into the body frame at EVERY stage with that stage's attitude
// (model_f<WorldWrench>).  ~600 / ~660 FP64 ops, 240 B (+ 48 B) in, 96 B (+ logs) out per instance.
// thruster_eval_kernel / plant_thruster_kernel<WW>: the same step behind the thruster stage (limits, per-instance gain / bias faults from an
// onset tick, a 6 x 6 propulsion matrix; brov_thruster_*), with or without the world wrench on top, and the stage alone.
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"
#include "plant_stages.hpp"   // wrench_at, thruster_stage, thruster_account

namespace brov {

__global__ __launch_bounds__(128) void wrench_eval_kernel(WrenchGen g, int B, long long tick, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double w[6];
    wrench_at(g, b, tick, w);
#pragma unroll
    for (int c = 0; c < 6; c++) out[(size_t)b * 6 + c] = w[c];
}

// x0 <- ERK4(x0, u0, p_plant, dt): the step immediately AFTER the hot path, the plant update of closed-loop Monte-Carlo
// roll-outs.  The same 12-state model the OCP uses (bluerov2.py:103-137) integrated over one control period with the first optimal input
// of the last solve, per-instance TRUE parameters (disturbance draw, model mismatch).  ~600 FP64 ops, 240 B in / 96 B out.
// Gather inputs -> plant_erk4 -> store, all three from bluerov2_model.hpp.
__global__ __launch_bounds__(128) void plant_kernel(double* __restrict__ x0, const brov_result* __restrict__ res, const double* __restrict__ pplant,
                             const double* __restrict__ prp, int rp_stride, int B, double dt, int substeps, double* __restrict__ xlog,
                             double* __restrict__ ulog) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[NX], u[NU];
    ModelPar m;
    Wrench w;
    plant_inputs(x0 + (size_t)b * NX, res[b].u0, pplant + (size_t)b * NP, prp, (size_t)b * rp_stride, x, u, m, w);
    plant_erk4(x, w, m, NoWorldWrench{}, dt, substeps);
    store_row(x0 + (size_t)b * NX, x);
    log_row(xlog, b, x);
    log_row(ulog, b, u);
}

// The same step under the wrench of generator g at `tick`, held over the tick like the reference's service call.  Its statements are those of
// plant_inputs / erk4_step / store_row written out, NOT calls of them: every form of this kernel that called them, or shared a templated
// body with plant_kernel, compiled to other code, and the one that was measured ran 2 ... 3 % slower per launch at B = 16384
// (profiles/plant_step_refactor_isa.txt, sections 3 and 6).  As it stands it is instruction for instruction the parent's kernel.  A change
// to the step is made in erk4_step (bluerov2_model.hpp), here, and in plant_step_wave (qp/fused.hpp).
__global__ __launch_bounds__(128) void plant_wrench_kernel(double* __restrict__ x0, const brov_result* __restrict__ res,
                                                           const double* __restrict__ pplant, const double* __restrict__ prp, int rp_stride, int B,
                                                           double dt, int substeps, double* __restrict__ xlog, double* __restrict__ ulog,
                                                           WrenchGen g, long long tick, double* __restrict__ wlog) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[NX], u[NU], k[NX], xs[NX], acc[NX], wv[6];
#pragma unroll
    for (int j = 0; j < NX; j++) x[j] = x0[(size_t)b * NX + j];
#pragma unroll
    for (int j = 0; j < NU; j++) u[j] = res[b].u0[j];
    const ModelPar m = make_par(pplant + (size_t)b * NP);
    Wrench w = make_wrench(u);
    if (prp) { w.k3 = prp[(size_t)b * rp_stride]; w.k4 = prp[(size_t)b * rp_stride + 1]; }   // 6-disturbance variant
    wrench_at(g, b, tick, wv);
    const WorldWrench ww = {wv[0], wv[1], wv[2], wv[3], wv[4], wv[5]};   // held over the tick, like the reference's service call
    const double h = dt / substeps;
    StagePoint sp;
    for (int s = 0; s < substeps; s++) {
        model_f(x, w, m, ww, k, sp);
#pragma unroll
        for (int j = 0; j < NX; j++) { acc[j] = x[j] + (h / 6.0) * k[j]; xs[j] = x[j] + 0.5 * h * k[j]; }
        model_f(xs, w, m, ww, k, sp);
#pragma unroll
        for (int j = 0; j < NX; j++) { acc[j] += (h / 3.0) * k[j]; xs[j] = x[j] + 0.5 * h * k[j]; }
        model_f(xs, w, m, ww, k, sp);
#pragma unroll
        for (int j = 0; j < NX; j++) { acc[j] += (h / 3.0) * k[j]; xs[j] = x[j] + h * k[j]; }
        model_f(xs, w, m, ww, k, sp);
#pragma unroll
        for (int j = 0; j < NX; j++) x[j] = acc[j] + (h / 6.0) * k[j];
    }
#pragma unroll
    for (int j = 0; j < NX; j++) x0[(size_t)b * NX + j] = x[j];
    if (xlog) {
#pragma unroll
        for (int j = 0; j < NX; j++) xlog[(size_t)b * NX + j] = x[j];
    }
    if (ulog) {
#pragma unroll
        for (int j = 0; j < NU; j++) ulog[(size_t)b * NU + j] = u[j];
    }
    if (wlog) {
#pragma unroll
        for (int c = 0; c < 6; c++) wlog[(size_t)b * 6 + c] = wv[c];
    }
}

__global__ __launch_bounds__(128) void thruster_eval_kernel(ThrusterPar T, ThrusterDev D, int B, long long tick, const double* __restrict__ commanded,
                                                            double* __restrict__ applied, double* __restrict__ wrench) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double t[6], a[6], g[6];
#pragma unroll
    for (int i = 0; i < 6; i++) t[i] = commanded[(size_t)b * 6 + i];
    thruster_stage(T, D, b, tick, t, a, g);
    store_row(applied + (size_t)b * 6, a);
    store_row(wrench + (size_t)b * 6, g);
}

// The plant step behind the thruster stage: gather -> stage -> plant_erk4 -> store / logs / statistics.  The wrench of the step is the
// stage's g = [X Y Z K M N] in place of make_wrench(u0); the roll / pitch moments of the 6-disturbance variant are ADDED to its k3, k4.
// WW = WorldWrench: the generator g at `tick` on top, evaluated and logged as plant_wrench_kernel does.  The `u` log stays the commanded input.
template <class WW>
__global__ __launch_bounds__(128) void plant_thruster_kernel(double* __restrict__ x0, const brov_result* __restrict__ res,
                                                             const double* __restrict__ pplant, const double* __restrict__ prp, int rp_stride, int B,
                                                             double dt, int substeps, double* __restrict__ xlog, double* __restrict__ ulog,
                                                             ThrusterPar T, ThrusterDev D, WrenchGen gen, long long tick, double* __restrict__ wlog) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[NX], u[NU], t[6], a[6], g[6];
#pragma unroll
    for (int j = 0; j < NX; j++) x[j] = x0[(size_t)b * NX + j];
#pragma unroll
    for (int j = 0; j < NU; j++) u[j] = res[b].u0[j];
#pragma unroll
    for (int i = 0; i < 6; i++) t[i] = res[b].thrust[i];
    const ModelPar m = make_par(pplant + (size_t)b * NP);
    thruster_stage(T, D, b, tick, t, a, g);
    thruster_account(T, D, b, t, a);
    Wrench w;
    w.k0 = g[0]; w.k1 = g[1]; w.k2 = g[2]; w.k3 = g[3]; w.k4 = g[4]; w.k5 = g[5];
    if (prp) { w.k3 += prp[(size_t)b * rp_stride]; w.k4 += prp[(size_t)b * rp_stride + 1]; }   // 6-disturbance variant
    if constexpr (std::is_same_v<WW, WorldWrench>) {
        double wv[6];
        wrench_at(gen, b, tick, wv);
        const WorldWrench ww = {wv[0], wv[1], wv[2], wv[3], wv[4], wv[5]};   // held over the tick
        log_row(wlog, b, wv);
        plant_erk4(x, w, m, ww, dt, substeps);
    } else {
        plant_erk4(x, w, m, NoWorldWrench{}, dt, substeps);
    }
    store_row(x0 + (size_t)b * NX, x);
    log_row(xlog, b, x);
    log_row(ulog, b, u);
}

// dst[b][c] = src[b * src_stride + col0 + c]: the disturbance estimate out of the observer's state for brov_closed_loop_dob's log
__global__ void gather_cols_kernel(const double* __restrict__ src, int B, int src_stride, int col0, int ncols, double* __restrict__ dst) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * ncols) return;
    const int b = t / ncols, c = t - b * ncols;
    dst[t] = src[(size_t)b * src_stride + col0 + c];
}

void launch_plant(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, int B, double dt, int substeps,
                  double* xlog, double* ulog, hipStream_t st) {
    hipLaunchKernelGGL(plant_kernel, dim3((B + 127) / 128), dim3(128), 0, st, x0, res, pplant, prp, rp_stride, B, dt, substeps, xlog, ulog);
}
void launch_plant_wrench(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, int B, double dt, int substeps,
                         double* xlog, double* ulog, const WrenchGen& g, long long tick, double* wlog, hipStream_t st) {
    hipLaunchKernelGGL(plant_wrench_kernel, dim3((B + 127) / 128), dim3(128), 0, st, x0, res, pplant, prp, rp_stride, B, dt, substeps, xlog, ulog,
                       g, tick, wlog);
}
void launch_wrench_eval(const WrenchGen& g, int B, long long tick, double* out, hipStream_t st) {
    hipLaunchKernelGGL(wrench_eval_kernel, dim3((B + 127) / 128), dim3(128), 0, st, g, B, tick, out);
}
void launch_plant_thruster(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, int B, double dt, int substeps,
                           double* xlog, double* ulog, const ThrusterPar& T, const ThrusterDev& D, const WrenchGen& g, long long tick, double* wlog,
                           hipStream_t st) {
    if (g.mode == BROV_WRENCH_OFF)
        hipLaunchKernelGGL(plant_thruster_kernel<NoWorldWrench>, dim3((B + 127) / 128), dim3(128), 0, st, x0, res, pplant, prp, rp_stride, B, dt,
                           substeps, xlog, ulog, T, D, g, tick, wlog);
    else
        hipLaunchKernelGGL(plant_thruster_kernel<WorldWrench>, dim3((B + 127) / 128), dim3(128), 0, st, x0, res, pplant, prp, rp_stride, B, dt,
                           substeps, xlog, ulog, T, D, g, tick, wlog);
}
void launch_thruster_eval(const ThrusterPar& T, const ThrusterDev& D, int B, long long tick, const double* commanded, double* applied, double* wrench,
                          hipStream_t st) {
    hipLaunchKernelGGL(thruster_eval_kernel, dim3((B + 127) / 128), dim3(128), 0, st, T, D, B, tick, commanded, applied, wrench);
}
void launch_gather_cols(const double* src, int B, int src_stride, int col0, int ncols, double* dst, hipStream_t st) {
    const int tot = B * ncols;
    hipLaunchKernelGGL(gather_cols_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, src, B, src_stride, col0, ncols, dst);
}

}  // namespace brov
