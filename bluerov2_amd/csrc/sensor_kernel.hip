// sensor_kernel.hip -- the sensor stage between the plant and the controller (brov_sensor_*): the MEASURED state ymeas [B][12] that the solve,
// the observer and the estimator read in place of the plant's true state while the stage is on.  The plant, the logs and the tracker keep
// the true state.  For channel c of instance b at measurement index m (the plant's tick counter), x the true value:
//   v = (x + bias[b][c]) + sigma[b][c] * n(b, m, c)
//   y = quant[c] > 0 ? rint(v / quant[c]) * quant[c] : v                        (a NaN passes through; rint: ties to even)
// every operation rounded on its own (rn_mul / rn_add of rounded_ops.hpp): both kernels and the numpy restatement of
// tests/sensor_restatement.py agree bit for bit.
// The noise n is counter-based and built from integers alone -- no libm on either side:
//   H(k) = splitmix64_finalise((seed ^ 0x53454E534F52) + (k + 1) * 0x9E3779B97F4A7C15),   k = b << 32 | m << 8 | c << 2 | j,   j = 0, 1, 2
//   S    = the sum of the twelve 16-bit fields of H(k | 0), H(k | 1), H(k | 2);    n = (S - 393210) / 65536     (exact)
// an Irwin-Hall(12) variate: variance 1 - 2^-32, bounded by +-6, kurtosis 2.9 (a Gaussian has 3).  The dropout draw of (b, m) is
// u = (H >> 11) * 2^-53 at the channel slot c = 12, j = 0: the fix is dropped iff dropout[b] > 0 && u < dropout[b].
// sensor_measure_kernel: one refresh of ymeas, regular or forced (see there).  sensor_eval_kernel: the stage alone.
// One lane per instance, FP64, no LDS, no scratch, no atomics; 480 B (a regular refresh: 688 B with the statistics) and up to 37 hashes
// per instance: launch-latency-sized at loop batch sizes, bound by HBM traffic at B = 262 144.
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "rounded_ops.hpp"

namespace brov {

// (sensor_hash and sensor_noise: rounded_ops.hpp, shared with the IMU/GPS stage of imu_kernel.hip, whose channel slots are 16..28)

// is the fix of (b, m) dropped?
__device__ __forceinline__ bool sensor_dropped(const SensorPar& P, const SensorDev& D, int b, int m) {
    const double p = D.dropout[b];
    if (!(p > 0.0)) return false;
    const double u = (double)(sensor_hash(P.seed, b, m, 12, 0) >> 11) * 0x1.0p-53;   // exact: 53 bits
    return u < p;
}

// the fresh sample of channel c for the true value x under this instance's bias and sigma of the channel
__device__ __forceinline__ double sensor_sample(const SensorPar& P, int b, int m, int c, double x, double bias, double sigma) {
#pragma clang fp contract(off)
    const double v = rn_add(rn_add(x, bias), rn_mul(sigma, sensor_noise(P.seed, b, m, c)));
    const double q = P.quant[c];
    return q > 0.0 ? rn_mul(rint(v / q), q) : v;
}

// ymeas <- one refresh from the true state x at index m.
//   regular: a dropped fix samples nothing; otherwise channel c takes its fresh sample iff m % period[c] == 0 and else keeps its value.  Then
//            the statistics: dropped[b] += drop, err_sq[b][c] += d * d with d = ymeas[c] - x[c] AFTER the refresh -- a held, stale value
//            counts as the error the controller really sees.
//   forced:  every channel takes its fresh sample, no dropout draw, the statistics are untouched.
__global__ __launch_bounds__(128) void sensor_measure_kernel(SensorPar P, SensorDev D, int B, int m, int forced, const double* __restrict__ x,
                                                             double* __restrict__ ymeas) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const bool drop = !forced && sensor_dropped(P, D, b, m);
    // the four rows of the instance up front, whether or not a channel is sampled: loads inside the per-channel branch would be twelve
    // dependent round trips to memory
    double xv[12], y[12], bi[12], sg[12];
#pragma unroll
    for (int c = 0; c < 12; c++) {
        xv[c] = x[(size_t)b * 12 + c]; y[c] = ymeas[(size_t)b * 12 + c];
        bi[c] = D.bias[(size_t)b * 12 + c]; sg[c] = D.sigma[(size_t)b * 12 + c];
    }
#pragma unroll
    for (int c = 0; c < 12; c++) {
        const bool take = forced || (!drop && m % P.period[c] == 0);
        if (take) y[c] = sensor_sample(P, b, m, c, xv[c], bi[c], sg[c]);
    }
#pragma unroll
    for (int c = 0; c < 12; c++) ymeas[(size_t)b * 12 + c] = y[c];
    if (forced) return;
    D.dropped[b] += drop ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 12; c++) {
        const double d = rn_add(y[c], -xv[c]);
        D.err_sq[(size_t)b * 12 + c] = rn_add(D.err_sq[(size_t)b * 12 + c], rn_mul(d, d));
    }
}

__global__ __launch_bounds__(128) void sensor_eval_kernel(SensorPar P, SensorDev D, int B, int m, const double* __restrict__ x, double* __restrict__ y,
                                                          int32_t* __restrict__ dropped) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
#pragma unroll
    for (int c = 0; c < 12; c++)
        y[(size_t)b * 12 + c] = sensor_sample(P, b, m, c, x[(size_t)b * 12 + c], D.bias[(size_t)b * 12 + c], D.sigma[(size_t)b * 12 + c]);
    if (dropped) dropped[b] = sensor_dropped(P, D, b, m) ? 1 : 0;
}

void launch_sensor_measure(const SensorPar& P, const SensorDev& D, int B, long long m, bool forced, const double* x, double* ymeas, hipStream_t st) {
    hipLaunchKernelGGL(sensor_measure_kernel, dim3((B + 127) / 128), dim3(128), 0, st, P, D, B, (int)m, forced ? 1 : 0, x, ymeas);
}
void launch_sensor_eval(const SensorPar& P, const SensorDev& D, int B, long long m, const double* x, double* y, int32_t* dropped, hipStream_t st) {
    hipLaunchKernelGGL(sensor_eval_kernel, dim3((B + 127) / 128), dim3(128), 0, st, P, D, B, (int)m, x, y, dropped);
}

}  // namespace brov
