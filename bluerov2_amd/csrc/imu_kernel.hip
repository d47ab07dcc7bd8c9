// imu_kernel.hip -- the IMU/GPS stage behind the plant (brov_imu_*): what the error-state filter (eskf_kernel.hip) reads -- a specific force,
// body rates, position fixes with their differenced velocity and an attitude -- made from the TRUE plant state at the sensors' own rates.
// Per instance b, after a plant step of length h to the true state x = (p, Euler angles, nu, rates) at measurement index m (the plant's counter):
//   R, q(phi, theta, psi)   from the Euler angles, as eskf_inputs_from_solver_kernel forms them (sincos_pio2; q from the half angles)
//   v_I = R nu;   a = R'((v_I - v_I,prev) / h - g_I),  g_I = (0, 0, -g)        the mean specific force of the step: a delta-velocity IMU
//   w   = (p, q, r)
//   a_m[k] = (a[k] + bias[b][k])     + sigma[b][k]     * n(b, m, 16 + k)
//   w_m[k] = (w[k] + bias[b][3 + k]) + sigma[b][3 + k] * n(b, m, 19 + k)
// n is the sensor stage's counter-based Irwin-Hall(12) variate (rounded_ops.hpp: the same hash, salt and key layout) at the channel slots
// 16..28: a sensor stage and an IMU stage with the same seed draw from disjoint counters.  A fix is DUE iff m % gps_every == 0 and DROPPED iff
// dropout[b] > 0 and u < dropout[b], u = (H >> 11) * 2^-53 at slot 28, j = 0;  fix[b] = due and not dropped.  With a fix:
//   gps_p[k] = x[k] + sigma[b][6 + k] * n(b, m, 22 + k)
//   gps_v    = (gps_p - gps_p,last) / (gps_every * h)        the constant nominal period: after a dropped fix the velocity is too large
//              (BROV_IMU_GPSV_ELAPSED: / ((m - m_last) * h) instead)
//   q_meas   = q(phi, theta, psi) * exp(sigma[b][9..11] . n(b, m, 25..27)), normalised;   gps_p,last and m_last move.
// Without a fix gps_p, gps_v and q_meas keep their values.  Every operation is rounded on its own (fp contract off; the sums that
// tests/imu_restatement.py restates bit for bit are written with rn_add / rn_mul).
// A FORCED refresh (restart): v_I,prev := the current v_I, so a is gravity alone; a fix is taken without a dropout draw, gps_v = 0; the
// statistics (samples, fixes taken, fixes dropped per instance) are untouched.
// imu_measure_kernel: one refresh of the stage's outputs and state.  imu_eval_kernel: the stage alone for given previous values.
// One lane per instance, FP64, no LDS, no scratch, no atomics; 296 B read and up to 168 B written per instance, up to 37 hashes.
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"   // sincos_pio2
#include "rounded_ops.hpp"

namespace brov {

constexpr int kImuSlotAcc = 16, kImuSlotGyro = 19, kImuSlotGps = 22, kImuSlotAtt = 25, kImuSlotDrop = 28;

struct ImuSample {
    double imu[6], gp[3], gv[3], qm[4], vI[3];
    bool fix, dropped;
};

// the sample of instance b at index m from the state x and the previous values (vp: v_I,prev; pl, ml: the last fix and its index, ml < 0: none)
__device__ __forceinline__ void imu_sample(const ImuPar& P, const ImuDev& D, int b, int m, bool forced, const double (&x)[12], const double (&vp)[3],
                                           const double (&pl)[3], int ml, ImuSample& o) {
#pragma clang fp contract(off)
    double sph, cph, sth, cth, sps, cps;
    sincos_pio2(x[3], &sph, &cph);
    sincos_pio2(x[4], &sth, &cth);
    sincos_pio2(x[5], &sps, &cps);
    const double R[9] = {cps * cth, -(sps * cph) + (cps * sth) * sph, sps * sph + (cps * cph) * sth,
                         sps * cth, cps * cph + (sph * sth) * sps,    -(cps * sph) + (sth * sps) * cph,
                         -sth,      cth * sph,                        cth * cph};
    double t[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.vI[k] = (R[k * 3] * x[6] + R[k * 3 + 1] * x[7]) + R[k * 3 + 2] * x[8];
        const double prev = forced ? o.vI[k] : vp[k];
        t[k] = (o.vI[k] - prev) / P.h + (k == 2 ? P.g : 0.0);      // - g_I
    }
    const double* sg = D.sigma + (size_t)b * 12;
    const double* bi = D.bias + (size_t)b * 6;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double a = (R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2];
        o.imu[k] = rn_add(rn_add(a, bi[k]), rn_mul(sg[k], sensor_noise(P.seed, b, m, kImuSlotAcc + k)));
        o.imu[3 + k] = rn_add(rn_add(x[9 + k], bi[3 + k]), rn_mul(sg[3 + k], sensor_noise(P.seed, b, m, kImuSlotGyro + k)));
    }
    const bool due = forced || m % P.gps_every == 0;
    bool drop = false;
    if (due && !forced) {
        const double p = D.dropout[b];
        if (p > 0.0) drop = (double)(sensor_hash(P.seed, b, m, kImuSlotDrop, 0) >> 11) * 0x1.0p-53 < p;   // exact: 53 bits
    }
    o.dropped = drop;
    o.fix = due && !drop;
    if (!o.fix) return;
    const bool none = forced || ml < 0;
    const double period = rn_mul((P.flags & BROV_IMU_GPSV_ELAPSED) ? (double)(m - ml) : (double)P.gps_every, P.h);
    double phi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        o.gp[k] = rn_add(x[k], rn_mul(sg[6 + k], sensor_noise(P.seed, b, m, kImuSlotGps + k)));
        o.gv[k] = none ? 0.0 : rn_add(o.gp[k], -pl[k]) / period;
        phi[k] = rn_mul(sg[9 + k], sensor_noise(P.seed, b, m, kImuSlotAtt + k));
    }
    double sh, ch, st2, ct2, sp2, cp2;
    sincos_pio2(0.5 * x[3], &sh, &ch);
    sincos_pio2(0.5 * x[4], &st2, &ct2);
    sincos_pio2(0.5 * x[5], &sp2, &cp2);
    const double q[4] = {(cp2 * ct2) * ch + (sp2 * st2) * sh, (cp2 * ct2) * sh - (sp2 * st2) * ch, (cp2 * st2) * ch + (sp2 * ct2) * sh,
                         (sp2 * ct2) * ch - (cp2 * st2) * sh};
    // exp(phi) = [cos(|phi| / 2), sin(|phi| / 2) / |phi| phi], below |phi|^2 = 2^-40 its series (the filter's q_exp)
    const double t2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2];
    const double tn = sqrt(t2);
    double sn, cs;
    sincos_pio2(0.5 * tn, &sn, &cs);
    const bool tiny = t2 < 0x1p-40;
    const double re = tiny ? 1.0 - t2 * 0.125 : cs;
    const double im = tiny ? 0.5 - t2 * (1.0 / 48.0) : sn / tn;
    const double e[4] = {re, im * phi[0], im * phi[1], im * phi[2]};
    const double r0 = ((q[0] * e[0] - q[1] * e[1]) - q[2] * e[2]) - q[3] * e[3], r1 = ((q[0] * e[1] + q[1] * e[0]) + q[2] * e[3]) - q[3] * e[2];
    const double r2 = ((q[0] * e[2] - q[1] * e[3]) + q[2] * e[0]) + q[3] * e[1], r3 = ((q[0] * e[3] + q[1] * e[2]) - q[2] * e[1]) + q[3] * e[0];
    const double in = 1.0 / sqrt(((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3);
    o.qm[0] = r0 * in; o.qm[1] = r1 * in; o.qm[2] = r2 * in; o.qm[3] = r3 * in;
}

// the sample's outputs: the IMU channels and the flag always, the fix's values where there is one
__device__ __forceinline__ void imu_store(const ImuOut& O, int b, const ImuSample& s) {
#pragma unroll
    for (int k = 0; k < 6; k++) O.imu[(size_t)b * 6 + k] = s.imu[k];
    O.fix[b] = s.fix ? 1 : 0;
    if (!s.fix) return;
#pragma unroll
    for (int k = 0; k < 3; k++) { O.gps_p[(size_t)b * 3 + k] = s.gp[k]; O.gps_v[(size_t)b * 3 + k] = s.gv[k]; }
#pragma unroll
    for (int k = 0; k < 4; k++) O.qm[(size_t)b * 4 + k] = s.qm[k];
}

__global__ __launch_bounds__(128) void imu_measure_kernel(ImuPar P, ImuDev D, ImuOut O, int B, int m, int forced, const double* __restrict__ x) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double xv[12], vp[3], pl[3];
#pragma unroll
    for (int c = 0; c < 12; c++) xv[c] = x[(size_t)b * 12 + c];
#pragma unroll
    for (int k = 0; k < 3; k++) { vp[k] = D.vprev[(size_t)b * 3 + k]; pl[k] = D.plast[(size_t)b * 3 + k]; }
    ImuSample s;
    imu_sample(P, D, b, m, forced != 0, xv, vp, pl, D.mlast[b], s);
    imu_store(O, b, s);
#pragma unroll
    for (int k = 0; k < 3; k++) D.vprev[(size_t)b * 3 + k] = s.vI[k];
    if (s.fix) {
#pragma unroll
        for (int k = 0; k < 3; k++) D.plast[(size_t)b * 3 + k] = s.gp[k];
        D.mlast[b] = m;
    }
    if (forced) return;
    D.stats[(size_t)b * 3] += 1;
    D.stats[(size_t)b * 3 + 1] += s.fix ? 1 : 0;
    D.stats[(size_t)b * 3 + 2] += s.dropped ? 1 : 0;
}

// the stage alone: a regular refresh's sample for the given previous values; without a fix gps_p, gps_v and q_meas of O are left as they are
__global__ __launch_bounds__(128) void imu_eval_kernel(ImuPar P, ImuDev D, ImuOut O, int B, int m, const double* __restrict__ x,
                                                       const double* __restrict__ vprev, const double* __restrict__ plast,
                                                       const int32_t* __restrict__ mlast) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double xv[12], vp[3], pl[3];
#pragma unroll
    for (int c = 0; c < 12; c++) xv[c] = x[(size_t)b * 12 + c];
#pragma unroll
    for (int k = 0; k < 3; k++) { vp[k] = vprev[(size_t)b * 3 + k]; pl[k] = plast[(size_t)b * 3 + k]; }
    ImuSample s;
    imu_sample(P, D, b, m, false, xv, vp, pl, mlast[b], s);
    imu_store(O, b, s);
}

void launch_imu_measure(const ImuPar& P, const ImuDev& D, const ImuOut& O, int B, long long m, bool forced, const double* x, hipStream_t st) {
    hipLaunchKernelGGL(imu_measure_kernel, dim3((B + 127) / 128), dim3(128), 0, st, P, D, O, B, (int)m, forced ? 1 : 0, x);
}
void launch_imu_eval(const ImuPar& P, const ImuDev& D, const ImuOut& O, int B, long long m, const double* x, const double* vprev, const double* plast,
                     const int32_t* mlast, hipStream_t st) {
    hipLaunchKernelGGL(imu_eval_kernel, dim3((B + 127) / 128), dim3(128), 0, st, P, D, O, B, (int)m, x, vprev, plast, mlast);
}

}  // namespace brov
