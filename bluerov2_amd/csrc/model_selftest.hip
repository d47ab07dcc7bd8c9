// model_selftest.hip -- test hook: the device model's building blocks alone (tests/test_gpu_model_exact.py checks them against a
// 60-digit reference, tests/model_exact.py).  Through a plant step an error of sincos_pio2 reaches x+ multiplied by h * v ~ 0.05; only a
// direct call shows it in units of the last place.  One lane per item:
//   a[i]          -> sincos_pio2(a[i])                                               out[i][0], out[i][1]
//   d[i]          -> rcp_nr(d[i])                                                    out[i][2]
//   in[i][0..40)  =  x[12] | u[4] | p[16] | world wrench[6] | roll / pitch moments[2]
//                 -> model_f<NoWorldWrench> (moments in, wrench ignored)             out[i][3 .. 15)
//                    model_f<WorldWrench>                                            out[i][15 .. 27)
// with make_par / make_wrench in front of model_f, as every plant has them.
#include <hip/hip_runtime.h>

#include "bluerov2_model.hpp"
#include "../../include/bluerov2_nmpc.h"

namespace brov {

constexpr int kSelftestIn = NX + NU + NP + 6 + 2, kSelftestOut = 3 + 2 * NX;

__global__ __launch_bounds__(64) void model_selftest_kernel(const double* __restrict__ a, const double* __restrict__ d,
                                                            const double* __restrict__ in, double* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double* o = out + (size_t)i * kSelftestOut;
    double sn, cs;
    sincos_pio2(a[i], &sn, &cs);
    o[0] = sn; o[1] = cs;
    o[2] = rcp_nr(d[i]);
    const double* r = in + (size_t)i * kSelftestIn;
    double x[NX], u[NU], f[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) x[j] = r[j];
#pragma unroll
    for (int j = 0; j < NU; j++) u[j] = r[NX + j];
    const ModelPar m = make_par(r + NX + NU);
    Wrench w = make_wrench(u);
    w.k3 = r[NX + NU + NP + 6]; w.k4 = r[NX + NU + NP + 7];
    const WorldWrench ww = {r[NX + NU + NP], r[NX + NU + NP + 1], r[NX + NU + NP + 2], r[NX + NU + NP + 3], r[NX + NU + NP + 4],
                            r[NX + NU + NP + 5]};
    StagePoint sp;
    model_f(x, w, m, NoWorldWrench{}, f, sp);
    store_row(o + 3, f);
    model_f(x, w, m, ww, f, sp);
    store_row(o + 3 + NX, f);
}

}  // namespace brov

// a, d: [n]; in: [n][40]; out: [n][27] (host pointers)
extern "C" int brov_selftest_model(const double* a, const double* d, const double* in, double* out, int n) {
    using namespace brov;
    if (!a || !d || !in || !out || n < 1) return BROV_ERR_ARG;
    const size_t nin = (size_t)n * (2 + kSelftestIn), nout = (size_t)n * kSelftestOut;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return BROV_ERR_NO_DEVICE;
    double* dev = nullptr;
    if (hipMalloc((void**)&dev, (nin + nout) * sizeof(double)) != hipSuccess) return BROV_ERR_ALLOC;
    double *da = dev, *dd = dev + n, *din = dev + 2 * (size_t)n, *dout = dev + nin;
    hipError_t e = hipMemcpy(da, a, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dd, d, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(din, in, (size_t)n * kSelftestIn * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(model_selftest_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, da, dd, din, dout, n);
        e = hipGetLastError();                                                  // the launch itself
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost);   // (waits for the kernel: its faults show here)
    hipFree(dev);
    return e == hipSuccess ? BROV_OK : BROV_ERR_HIP;
}
