// delay_kernel.hip -- the delay stage of the solver's plant (include/bluerov2_nmpc.h, brov_delay_*): the command solved at tick k acts on the
// vehicle `delay[b]` plant steps later, and a controller that knows its nominal delay predicts its measurement through the commands still
// under way before it solves.
// delay_shift_kernel: ahead of every plant step.  Per instance a ring of the last D commanded records (u0[4] | thrust[6], ten doubles a slot,
// [B][D][10]) indexed by the stage's own step count n.  It reads the commanded record c(n) = res[b], forms the applied record a(n) -- c(n) at
// delay 0, else slot (n - delay[b]) mod D, zeros while n < delay[b]; the read comes before the write --, writes c(n) into slot n mod D and
// applied[b] = res[b] with u0 and thrust replaced by a(n); a `u` log row gets the COMMANDED u0.  The plant kernels (plant_wrench.hip,
// plant_current.hip) then read `applied` in place of `res`: they read nothing of a record but u0 and thrust.  Copies only: bit-reproducible
// against tests/delay_restatement.py.
// delay_predict_kernel: ahead of every solve while comp > 0.  x^ = Phi(... Phi(Phi(y, c(n - comp)), c(n - comp + 1)) ..., c(n - 1)), Phi one
// ERK4 step over dt_pred (plant_erk4 of bluerov2_model.hpp, one substep) with the controller's own stage-0 parameters and, 6-disturbance
// variant, its roll / pitch moments; the inputs are the ring's u0 entries, oldest first, zeros for steps before the first.
// Both: one lane per instance, 128-thread blocks, FP64, no LDS, no scratch; comp, dt_pred, n and D are wave-uniform kernel arguments.
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"

namespace brov {

constexpr int kDelayRec = 10;   // doubles per ring slot: u0[4] | thrust[6]

__global__ __launch_bounds__(128) void delay_shift_kernel(const brov_result* __restrict__ res, brov_result* __restrict__ applied,
                                                          const int32_t* __restrict__ delay, double* __restrict__ ring, int D, long long n, int B,
                                                          double* __restrict__ ulog) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    brov_result r = res[b];
    double c[kDelayRec], a[kDelayRec];
#pragma unroll
    for (int j = 0; j < 4; j++) c[j] = r.u0[j];
#pragma unroll
    for (int j = 0; j < 6; j++) c[4 + j] = r.thrust[j];
    double* q = ring + (size_t)b * D * kDelayRec;
    int d = delay[b];
    d = d < 0 ? 0 : (d > D - 1 ? D - 1 : d);   // (the host has checked 0 <= delay[b] <= D - 1: no slot outside the ring whatever the buffer holds)
    if (d == 0) {
#pragma unroll
        for (int j = 0; j < kDelayRec; j++) a[j] = c[j];
    } else if (n < d) {
#pragma unroll
        for (int j = 0; j < kDelayRec; j++) a[j] = 0.0;
    } else {
        const double* src = q + (size_t)((n - d) % D) * kDelayRec;
#pragma unroll
        for (int j = 0; j < kDelayRec; j++) a[j] = src[j];
    }
    double* dst = q + (size_t)(n % D) * kDelayRec;
#pragma unroll
    for (int j = 0; j < kDelayRec; j++) dst[j] = c[j];
#pragma unroll
    for (int j = 0; j < 4; j++) r.u0[j] = a[j];
#pragma unroll
    for (int j = 0; j < 6; j++) r.thrust[j] = a[4 + j];
    applied[b] = r;
    if (ulog) {
#pragma unroll
        for (int j = 0; j < 4; j++) ulog[(size_t)b * 4 + j] = c[j];
    }
}

__global__ __launch_bounds__(128) void delay_predict_kernel(const double* __restrict__ y, const double* __restrict__ par, int par_stride,
                                                            const double* __restrict__ prp, int rp_stride, const double* __restrict__ ring, int D,
                                                            long long n, int comp, double dt_pred, double* __restrict__ xhat, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[NX], u[NU];
#pragma unroll
    for (int j = 0; j < NX; j++) x[j] = y[(size_t)b * NX + j];
    const ModelPar m = make_par(par + (size_t)b * par_stride);
    double k3 = 0.0, k4 = 0.0;
    if (prp) { k3 = prp[(size_t)b * rp_stride]; k4 = prp[(size_t)b * rp_stride + 1]; }   // 6-disturbance variant
    const double* q = ring + (size_t)b * D * kDelayRec;
    for (int i = 0; i < comp; i++) {
        const long long step = n - comp + i;   // wave-uniform: the commanded record of that step, zeros before the first
        if (step >= 0) {
            const double* src = q + (size_t)(step % D) * kDelayRec;
#pragma unroll
            for (int j = 0; j < NU; j++) u[j] = src[j];
        } else {
#pragma unroll
            for (int j = 0; j < NU; j++) u[j] = 0.0;
        }
        Wrench w = make_wrench(u);
        w.k3 = k3; w.k4 = k4;
        plant_erk4(x, w, m, NoWorldWrench{}, dt_pred, 1);
    }
    store_row(xhat + (size_t)b * NX, x);
}

void launch_delay_shift(const brov_result* res, brov_result* applied, const int32_t* delay, double* ring, int D, long long n, int B, double* ulog,
                        hipStream_t st) {
    hipLaunchKernelGGL(delay_shift_kernel, dim3((B + 127) / 128), dim3(128), 0, st, res, applied, delay, ring, D, n, B, ulog);
}
void launch_delay_predict(const double* y, const double* par, int par_stride, const double* prp, int rp_stride, const double* ring, int D, long long n,
                          int comp, double dt_pred, double* xhat, int B, hipStream_t st) {
    hipLaunchKernelGGL(delay_predict_kernel, dim3((B + 127) / 128), dim3(128), 0, st, y, par, par_stride, prp, rp_stride, ring, D, n, comp, dt_pred,
                       xhat, B);
}

}  // namespace brov
