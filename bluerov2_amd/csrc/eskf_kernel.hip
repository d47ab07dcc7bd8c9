// eskf_kernel.hip -- batched error-state Kalman filter with IMU disturbance observer and its C ABI (include/bluerov2_nmpc_eskf.h, brov_eskf_*).
// B independent copies of the reference's bluerov2_states nodelet (src/Eskf.cpp: predict :97-158, update :197-306, inject :320-332;
// Dynamics.cpp; Config.cpp): nominal state [p | v | q | b_g | b_a | g_I | xi] (22), covariance over the 21 error states, whose last three are the
// body-frame disturbance force the "patty" DOB node and the consolidated controller's DOMPC mode take from /disturbance.  The formulas stand in
// the header; tests/eskf_exact.py restates them at 60 digits.
//
// One kernel body, eskf_tick_kernel<UPDATE>: predict only, or predict followed by update.  Layout: one filter per 32 lanes (two per wave, one
// wave per block), lane i < 21 owns ROW i of P in registers, P also lies in LDS (441 doubles per filter) where the other lanes read it:
//   * F = I + six 3 x 3 blocks.  B = P F' only mixes COLUMNS 0..8 of a row: the lane's own registers.  F B only mixes ROWS 0..8: nine lanes read
//     up to seven rows of B out of LDS, the others keep theirs.  0.6 k multiply-adds per filter where the dense products have 18.5 k.
//   * the result is written back with its upper triangle mirrored: P_pred is exactly symmetric, in LDS and in every lane's row.
//   * H is a signed row selection: S is a signed 12 x 12 gather from P plus diag(R12) -- lane a < 12 owns row a --, P H' is twelve signed entries of
//     the lane's own row.  S is eliminated without row exchanges (S = L D L', the pivot row goes through LDS, every lane keeps the reciprocals
//     of the pivots): 12 steps.  Lane i then solves S z = (P H')[i,:]' for row i of the gain by two substitutions out of the factor in LDS,
//     forms dx_i = z . y and its row of P - Kal (P H')' from the twelve selected rows of P_pred in LDS.
//   * the nominal state (a few hundred operations: two quaternion exponentials, a logarithm, three rotation matrices) is carried by every lane
//     of the filter redundantly: no broadcast, no divergence; lane 0 writes it.
// P is read once and written once per tick, in 8-byte pieces 32 lanes wide: 2 x 3528 B, with x 2 x 176 B, inputs 176 B and outputs 84 B 7.5 KB per
// update against ~6 k multiply-adds: by bytes an HBM kernel.  A filter never reads another filter's registers or LDS: its result does not depend
// on its position in the batch or on what its wave neighbour holds.  DESIGN.md section 4.4b has the resources and the measurements.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "bluerov2_model.hpp"
#include "bluerov2_nmpc.h"

namespace brov {

constexpr int SN = 21, SX = 22, SY = 12;
constexpr int kEskfFilters = 2;                          // per wave: 32 lanes each
constexpr int kEskfLds = SN * SN + SY * SY + SN + SX + SY;   // doubles per filter: P, the factor of S, dx, the predicted state, the innovation
constexpr double kEskfSeries = 0x1p-40;                  // |phi|^2 below which exp and log take their series

struct EskfConst {
    double dt, mass, mzg, g, wb, vel_inject, inv_cc, inv_rc;   // mzg = m ZG, wb = m g - bouyancy
    double am[3], Dl[3], Dnl[3], K3[18], Q[SN], R12[SY];
    int inject, pad;
};
struct EskfArgs {
    const EskfConst* c;   // DEVICE: Q and R12 are indexed by lane
    int B;
    double* x;            // [B][22]
    double* P;            // [B][21][21]
    const double *imu, *gps_p, *gps_v, *qm, *thrust;   // [B][6], [B][3], [B][3], [B][4], [B][6]; the last four are not read by the predict-only tick
    double *xi, *xw, *mp; // [B][3], [B][3], [B][4]
    int* status;          // [B]
};

__device__ __forceinline__ void q_rot(const double (&q)[4], double (&R)[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}
// a * b, normalised
__device__ __forceinline__ void q_mul_unit(const double (&a)[4], const double (&b)[4], double (&o)[4]) {
    const double t0 = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], t1 = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    const double t2 = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], t3 = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
    const double in = 1.0 / sqrt(t0 * t0 + t1 * t1 + t2 * t2 + t3 * t3);
    o[0] = t0 * in; o[1] = t1 * in; o[2] = t2 * in; o[3] = t3 * in;
}
__device__ __forceinline__ void q_unit(const double* q, double (&o)[4]) {
    const double in = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    o[0] = q[0] * in; o[1] = q[1] * in; o[2] = q[2] * in; o[3] = q[3] * in;
}
// exp(phi) = [cos(t / 2), sin(t / 2) / t phi], t = |phi|
__device__ __forceinline__ void q_exp(double p0, double p1, double p2, double (&o)[4]) {
    const double t2 = p0 * p0 + p1 * p1 + p2 * p2;
    const double t = sqrt(t2);
    double sn, cs;
    sincos_pio2(0.5 * t, &sn, &cs);
    const bool tiny = t2 < kEskfSeries;
    const double re = tiny ? 1.0 - t2 * 0.125 : cs;
    const double im = tiny ? 0.5 - t2 * (1.0 / 48.0) : sn / t;
    o[0] = re; o[1] = im * p0; o[2] = im * p1; o[3] = im * p2;
}
// log(q) = 2 atan(n / w) / n v, n = |v|: atan, not atan2 -- q and -q have the same logarithm
__device__ __forceinline__ void q_log(const double (&q)[4], double (&o)[3]) {
    const double w = q[0];
    const double n2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const double n = sqrt(n2);
    const double big = (w == 0.0) ? 3.14159265358979323846 / n : 2.0 * atan(n / w) / n;
    const double k = (n2 < kEskfSeries) ? 2.0 / w - 2.0 * n2 / (3.0 * w * w * w) : big;
    o[0] = k * q[1]; o[1] = k * q[2]; o[2] = k * q[3];
}

// entry a of H's row selection: error state and sign
__host__ __device__ constexpr int eskf_hsel(int a) { return a < 9 ? a : a + 9; }
__host__ __device__ constexpr double eskf_hsgn(int a) { return a < 9 ? 1.0 : -1.0; }

// the lane's row into LDS, the part left of the diagonal back from the column above it, the row into LDS again: P exactly symmetric (its upper
// triangle mirrored over the lower one), in LDS and in the rows.  Straight-line code: lanes 21..31 write what lane 20 writes
__device__ __forceinline__ void eskf_mirror(double* Pm, double (&row)[SN], int i) {
    __syncthreads();   // every read of the old P is done
#pragma unroll
    for (int j = 0; j < SN; j++) Pm[i * SN + j] = row[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SN; j++) {
        const double t = Pm[j * SN + i];
        row[j] = (j >= i) ? row[j] : t;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SN; j++) Pm[i * SN + j] = row[j];
    __syncthreads();
}

template <bool UPDATE>
__global__ __launch_bounds__(64, 2) void eskf_tick_kernel(EskfArgs A) {
    __shared__ double sm[kEskfFilters * kEskfLds];
    const EskfConst& c = *A.c;
    const int f = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int inst0 = blockIdx.x * kEskfFilters + f;
    const bool live = inst0 < A.B;
    const int inst = live ? inst0 : A.B - 1;       // a dead half-wave repeats the last filter and writes nothing
    const int i = l < SN ? l : SN - 1;             // lanes 21..31 repeat row 20: the same values to the same LDS addresses
    double* Pm = sm + f * kEskfLds;
    double* U = Pm + SN * SN;
    double* dxs = U + SY * SY;
    double* xs = dxs + SN;
    double* ys = xs + SX;
    const double dt = c.dt;

    // ---- P -> LDS, 32 lanes wide; the nominal state and the IMU sample into every lane
    double* pg = A.P + (size_t)inst * (SN * SN);
#pragma unroll
    for (int m = 0; m < (SN * SN + 31) / 32; m++) {
        const int e = m * 32 + l;
        if (e < SN * SN) Pm[e] = pg[e];
    }
    double x[SX], a[3], w[3];
    {
        const double* xg = A.x + (size_t)inst * SX;
#pragma unroll
        for (int j = 0; j < SX; j++) x[j] = xg[j];
        const double* ig = A.imu + (size_t)inst * 6;
#pragma unroll
        for (int k = 0; k < 3; k++) { a[k] = ig[k] - x[13 + k]; w[k] = ig[3 + k] - x[10 + k]; }
    }
    __syncthreads();
    double row[SN];
#pragma unroll
    for (int j = 0; j < SN; j++) row[j] = Pm[i * SN + j];

    // ---- predict: the nominal state (Eskf.cpp:109-133) ...
    double q[4], M1[9], M2[9], E[9];
    {
        double q0[4], R[9], qe[4];
        q_unit(&x[6], q0);
        q_rot(q0, R);
        const double Ra[3] = {R[0] * a[0] + R[1] * a[1] + R[2] * a[2], R[3] * a[0] + R[4] * a[1] + R[5] * a[2], R[6] * a[0] + R[7] * a[1] + R[8] * a[2]};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double g = x[16 + k];
            x[k] = x[k] + x[3 + k] * dt + 0.5 * Ra[k] * dt * dt + 0.5 * g * dt * dt;
            x[3 + k] = x[3 + k] + Ra[k] * dt + g * dt;
        }
        q_exp(w[0] * dt, w[1] * dt, w[2] * dt, qe);
        q_mul_unit(q0, qe, q);
        // ... and the blocks of F (:150-157), from the NEW attitude
        q_rot(q, R);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            M1[r * 3 + 0] = -(R[r * 3 + 1] * a[2] - R[r * 3 + 2] * a[1]) * dt;
            M1[r * 3 + 1] = -(R[r * 3 + 2] * a[0] - R[r * 3 + 0] * a[2]) * dt;
            M1[r * 3 + 2] = -(R[r * 3 + 0] * a[1] - R[r * 3 + 1] * a[0]) * dt;
#pragma unroll
            for (int k = 0; k < 3; k++) M2[r * 3 + k] = -R[r * 3 + k] * dt;
        }
        q_exp(-(w[0] * dt), -(w[1] * dt), -(w[2] * dt), qe);
        q_rot(qe, E);
    }
    // ---- B = P F': columns 0..8 of the lane's own row
    {
        double t0[3], t1[3], t2[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            t0[r] = fma(dt, row[3 + r], row[r]);
            double s = fma(dt, row[15 + r], row[3 + r]), e = -dt * row[9 + r];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                s = fma(M1[r * 3 + k], row[6 + k], s);
                s = fma(M2[r * 3 + k], row[12 + k], s);
                e = fma(E[r * 3 + k], row[6 + k], e);
            }
            t1[r] = s; t2[r] = e;
        }
#pragma unroll
        for (int r = 0; r < 3; r++) { row[r] = t0[r]; row[3 + r] = t1[r]; row[6 + r] = t2[r]; }
    }
    __syncthreads();   // every lane has its row of P out of LDS
#pragma unroll
    for (int j = 0; j < SN; j++) Pm[i * SN + j] = row[j];      // (lanes 21..31: what lane 20 writes)
    __syncthreads();
    // ---- P_pred = F B + diag(Q): rows 0..8; the coefficients of the lane's row of F are selected, not indexed
    if (i < 9) {
        const int grp = i / 3, r = i - 3 * grp;
        double ca[3], cb[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double m1 = r == 0 ? M1[k] : (r == 1 ? M1[3 + k] : M1[6 + k]);
            const double m2 = r == 0 ? M2[k] : (r == 1 ? M2[3 + k] : M2[6 + k]);
            const double ee = r == 0 ? E[k] : (r == 1 ? E[3 + k] : E[6 + k]);
            ca[k] = grp == 1 ? m1 : (grp == 2 ? ee : 0.0);
            cb[k] = grp == 1 ? m2 : 0.0;
        }
        const double d = grp == 2 ? -dt : dt;
        const int rd = grp == 0 ? 3 + r : (grp == 1 ? 15 + r : 9 + r);
#pragma unroll
        for (int j = 0; j < SN; j++) {
            double s = grp == 2 ? 0.0 : row[j];
            s = fma(d, Pm[rd * SN + j], s);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                s = fma(ca[k], Pm[(6 + k) * SN + j], s);
                s = fma(cb[k], Pm[(12 + k) * SN + j], s);
            }
            row[j] = s;
        }
    }
    {
        const double qi = c.Q[i];
#pragma unroll
        for (int j = 0; j < SN; j++) row[j] += (j == i) ? qi : 0.0;
    }
    eskf_mirror(Pm, row, i);
#pragma unroll
    for (int k = 0; k < 4; k++) x[6 + k] = q[k];

    bool ok = true;
    if constexpr (UPDATE) {
        // ---- innovation (:203-272), every lane
        {
            double y[SY], qm[4], R[9], Rm[9];
            q_unit(A.qm + (size_t)inst * 4, qm);
            q_rot(q, R);
            q_rot(qm, Rm);
            const double* gp = A.gps_p + (size_t)inst * 3;
            const double* gv = A.gps_v + (size_t)inst * 3;
            const double* tg = A.thrust + (size_t)inst * 6;
            double th[6];
#pragma unroll
            for (int k = 0; k < 6; k++) th[k] = tg[k];
            const double qc[4] = {q[0], -q[1], -q[2], -q[3]};
            double dq[4], att[3];
            q_mul_unit(qc, qm, dq);
            q_log(dq, att);
            const double mrb[3] = {c.mass * a[0] + c.mzg * w[1], c.mass * a[1] - c.mzg * w[0], c.mass * a[2]};
#pragma unroll
            for (int k = 0; k < 3; k++) {
                y[k] = gp[k] - x[k];
                y[3 + k] = gv[k] - x[3 + k];
                y[6 + k] = att[k];
                const double vB = R[k] * x[3] + R[3 + k] * x[4] + R[6 + k] * x[5];          // R' v
                const double gB = -c.g * Rm[6 + k];                                        // R(q_meas)' (0, 0, -g)
                const double ma = c.am[k] * (a[k] + gB);
                const double d3 = (-c.Dl[k] - c.Dnl[k] * fabs(vB)) * vB;
                const double g3 = -c.wb * R[6 + k];   // (m g - b) [sin th, -cos th sin ph, -cos th cos ph] = -(m g - b) (row 2 of R)
                double tau = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) tau += c.K3[k * 6 + m] * th[m];
                y[9 + k] = tau - (mrb[k] - x[19 + k] + ma + d3 + g3);
            }
            // the predicted state and the innovation wait in LDS (every lane of the filter writes the same values) while the registers hold
            // the rows of S and of the gain
#pragma unroll
            for (int j = 0; j < SX; j++) xs[j] = x[j];
#pragma unroll
            for (int b = 0; b < SY; b++) ys[b] = y[b];
        }
        // ---- S = H P H' + diag(R12): lane a < 12 gathers row a; elimination without row exchanges, the pivot row through LDS
        double ipk[SY];
        {
            const int as = l < SY ? l : SY - 1;      // lanes 12..31 repeat row 11: the same values to the same addresses
            const int ha = eskf_hsel(as);
            const double sa = eskf_hsgn(as), r12 = c.R12[as];
            double srow[SY];
#pragma unroll
            for (int b = 0; b < SY; b++) srow[b] = (sa * eskf_hsgn(b)) * Pm[ha * SN + eskf_hsel(b)] + ((b == as) ? r12 : 0.0);
            // step k: every lane puts its row as it stands into LDS (rows <= k are final: the factor), the pivot row comes back to all, rows
            // below it are updated -- selected, not branched: straight-line code between the barriers
#pragma unroll
            for (int k = 0; k < SY; k++) {
#pragma unroll
                for (int j = k; j < SY; j++) U[as * SY + j] = srow[j];
                __syncthreads();
                const double pk = U[k * SY + k];
                ok = ok && (pk > 0.0) && (pk < 1e300);
                ipk[k] = 1.0 / pk;
                const double fk = srow[k] * ipk[k];
#pragma unroll
                for (int j = k + 1; j < SY; j++) {
                    const double t = fma(-fk, U[k * SY + j], srow[j]);
                    srow[j] = (as > k) ? t : srow[j];
                }
            }
        }
        // ---- row i of the gain: S z = (P H')[i,:]', two substitutions; dx_i; row i of P - Kal (P H')'
        double dxi = 0.0;
        if (ok) {
            double z[SY], t[SY];
#pragma unroll
            for (int b = 0; b < SY; b++) {
                double s = eskf_hsgn(b) * row[eskf_hsel(b)];
#pragma unroll
                for (int k = 0; k < b; k++) s = fma(-U[k * SY + b], t[k], s);
                z[b] = s; t[b] = s * ipk[b];
            }
#pragma unroll
            for (int b = SY - 1; b >= 0; b--) {
                double s = z[b];
#pragma unroll
                for (int j = b + 1; j < SY; j++) s = fma(-U[b * SY + j], z[j], s);
                z[b] = s * ipk[b];
            }
#pragma unroll
            for (int b = 0; b < SY; b++) dxi = fma(z[b], ys[b], dxi);
#pragma unroll
            for (int b = 0; b < SY; b++) {
                const double zb = -eskf_hsgn(b) * z[b];
#pragma unroll
                for (int j = 0; j < SN; j++) row[j] = fma(zb, Pm[eskf_hsel(b) * SN + j], row[j]);
            }
        }
        dxs[i] = dxi;
        eskf_mirror(Pm, row, i);   // (its first barrier also puts dxs in front of the reads below)
        // ---- inject (:320-332)
#pragma unroll
        for (int j = 0; j < SX; j++) x[j] = xs[j];
        if (ok) {
            const double q[4] = {x[6], x[7], x[8], x[9]};
            double dx[SN];
#pragma unroll
            for (int j = 0; j < SN; j++) dx[j] = dxs[j];
            double qe[4], qn[4];
            q_exp(dx[6], dx[7], dx[8], qe);
            q_mul_unit(q, qe, qn);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                x[k] += dx[k];
                x[3 + k] += c.vel_inject * dx[3 + k];
                x[19 + k] += dx[18 + k];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) x[6 + k] = qn[k];
            if (c.inject) {
#pragma unroll
                for (int k = 0; k < 9; k++) x[10 + k] += dx[9 + k];
            }
        }
    }
    // ---- out: P 32 lanes wide out of LDS, the state and the outputs by lane 0
    if (live) {
#pragma unroll
        for (int m = 0; m < (SN * SN + 31) / 32; m++) {
            const int e = m * 32 + l;
            if (e < SN * SN) pg[e] = Pm[e];
        }
        if (l == 0) {
            double* xg = A.x + (size_t)inst * SX;
            bool fin = true;
#pragma unroll
            for (int j = 0; j < SX; j++) { xg[j] = x[j]; fin = fin && (fabs(x[j]) < 1e300); }
            const double qf[4] = {x[6], x[7], x[8], x[9]};
            double R[9];
            q_rot(qf, R);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                A.xi[(size_t)inst * 3 + k] = x[19 + k];
                A.xw[(size_t)inst * 3 + k] = R[k * 3] * x[19] + R[k * 3 + 1] * x[20] + R[k * 3 + 2] * x[21];
            }
            double* mp = A.mp + (size_t)inst * 4;
            mp[0] = x[19] * c.inv_cc; mp[1] = x[20] * c.inv_cc; mp[2] = x[21] * c.inv_rc; mp[3] = 0.0;
            A.status[inst] = !ok ? 1 : (fin ? 0 : 2);
        }
    }
}

// the filter's inputs from the controller's view of the plant (one lane per filter): attitude quaternion and R from the Euler angles,
// v_I = R nu, a_m = R'((v_I - v_I,prev) / dt - g_I), w_m = (p, q, r), gps_p = (x, y, z), gps_v = (gps_p - gps_p,prev) / gps_dt; thrust = the
// allocation of u0 with the OCP model's rotor constant, as ekf_inputs_from_solver_kernel has it.  first: the previous values are the current ones
__global__ void eskf_inputs_from_solver_kernel(int B, double dt, double gps_dt, double g, double inv_rc, int first, const double* __restrict__ x0,
                                               const brov_result* __restrict__ res, double* __restrict__ vprev, double* __restrict__ pprev,
                                               double* __restrict__ imu, double* __restrict__ gps_p, double* __restrict__ gps_v,
                                               double* __restrict__ qm, double* __restrict__ thrust) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* xs = x0 + (size_t)b * 12;
    double sph, cph, sth, cth, sps, cps;
    sincos_pio2(xs[3], &sph, &cph);
    sincos_pio2(xs[4], &sth, &cth);
    sincos_pio2(xs[5], &sps, &cps);
    const double R[9] = {cps * cth, -sps * cph + cps * sth * sph, sps * sph + cps * cph * sth,
                         sps * cth, cps * cph + sph * sth * sps,  -cps * sph + sth * sps * cph,
                         -sth,      cth * sph,                    cth * cph};
    double vI[3], t[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        vI[k] = R[k * 3] * xs[6] + R[k * 3 + 1] * xs[7] + R[k * 3 + 2] * xs[8];
        const double vp = first ? vI[k] : vprev[(size_t)b * 3 + k];
        const double pp = first ? xs[k] : pprev[(size_t)b * 3 + k];
        t[k] = (vI[k] - vp) / dt + (k == 2 ? g : 0.0);      // - g_I, g_I = (0, 0, -g)
        gps_p[(size_t)b * 3 + k] = xs[k];
        gps_v[(size_t)b * 3 + k] = (xs[k] - pp) / gps_dt;
        vprev[(size_t)b * 3 + k] = vI[k];
        pprev[(size_t)b * 3 + k] = xs[k];
        imu[(size_t)b * 6 + 3 + k] = xs[9 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) imu[(size_t)b * 6 + k] = R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2];
    double sh, ch, st2, ct2, sp2, cp2;
    sincos_pio2(0.5 * xs[3], &sh, &ch);
    sincos_pio2(0.5 * xs[4], &st2, &ct2);
    sincos_pio2(0.5 * xs[5], &sp2, &cp2);
    double* qo = qm + (size_t)b * 4;
    qo[0] = cp2 * ct2 * ch + sp2 * st2 * sh;
    qo[1] = cp2 * ct2 * sh - sp2 * st2 * ch;
    qo[2] = cp2 * st2 * ch + sp2 * ct2 * sh;
    qo[3] = sp2 * ct2 * ch - cp2 * st2 * sh;
    const double u0 = res[b].u0[0], u1 = res[b].u0[1], u2 = res[b].u0[2], u3 = res[b].u0[3];
    double* th = thrust + (size_t)b * 6;
    th[0] = (-u0 + u1 + u3) * inv_rc;
    th[1] = (-u0 - u1 - u3) * inv_rc;
    th[2] = (u0 + u1 - u3) * inv_rc;
    th[3] = (u0 - u1 + u3) * inv_rc;
    th[4] = (-u2) * inv_rc;
    th[5] = (-u2) * inv_rc;
}

// p[0..3] of every stage of instance b := mpc_p of instance b (bluerov2_dob_patty.cpp:352-358); p[4..15] stay
__global__ void eskf_apply_kernel(int B, int stages, const double* __restrict__ mp, double* __restrict__ par) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B * stages) return;
    const int b = k / stages;
    double* p = par + (size_t)k * 16;
#pragma unroll
    for (int j = 0; j < 4; j++) p[j] = mp[(size_t)b * 4 + j];
}

}  // namespace brov

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
#include "host_common.hpp"

using namespace brov;

static thread_local std::string g_eskf_err;
#define HIPCHK(call) BROV_HIPCHK(g_eskf_err, call)

struct brov_eskf {
    int device = 0, B = 0;
    brov_eskf_params par{};
    EskfConst c{};
    EskfConst* cdev = nullptr;
    double *x = nullptr, *P = nullptr, *imu = nullptr, *gps_p = nullptr, *gps_v = nullptr, *qm = nullptr, *thrust = nullptr, *xi = nullptr,
           *xw = nullptr, *mp = nullptr, *vprev = nullptr, *pprev = nullptr;
    int* status = nullptr;
    bool first = true;   // no previous velocity and position yet: the next update_from_solver takes them equal to the current ones
    hipStream_t last_stream = nullptr;
    KernelTimer timer;   // around the last tick
    DeviceAllocs mem;
};

static int refuse(const char* who, const std::string& why) {
    g_eskf_err = std::string(who) + ": " + why;
    return BROV_ERR_ARG;
}

extern "C" const char* brov_eskf_last_error(void) { return g_eskf_err.c_str(); }

extern "C" void brov_eskf_default_params(brov_eskf_params* p) {
    // ImuDo.h:101-110; Config.cpp:128-154,175-180; launch/config/imudo.yaml; Eskf.cpp:103,184
    static const double am[6] = {1.7182, 0, 5.468, 0, 1.2481, 0.4006};
    static const double dl[6] = {-11.7391, -20, -31.8678, -25, -44.9085, -5};
    static const double dnl[6] = {-18.18, -21.66, -36.99, -1.55, -1.55, -1.55};
    static const double K[36] = {
        0.7071067811847433,   0.7071067811847433,    -0.7071067811919605, -0.7071067811919605,  0.0,                   0.0,
        0.7071067811883519,   -0.7071067811883519,   0.7071067811811348,  -0.7071067811811348,  0.0,                   0.0,
        0,                    0,                     0,                   0,                    1,                     1,
        0.051265241636155506, -0.05126524163615552,  0.05126524163563227, -0.05126524163563227, -0.11050000000000001,  0.11050000000000003,
        -0.05126524163589389, -0.051265241635893896, 0.05126524163641713, 0.05126524163641713,  -0.002499999999974481, -0.002499999999974481,
        0.16652364696949604,  -0.16652364696949604,  -0.17500892834341342, 0.17500892834341342, 0.0,                   0.0};
    static const double r12[4] = {0.01, 0.02, 0.0006, 0.012};
    std::memset(p, 0, sizeof(*p));
    p->dt = 1.0 / 50.0; p->gps_dt = 1.0 / 30.0;
    p->mass = 11.26; p->ZG = 0.02; p->g = 9.81; p->bouyancy = 0.661618;
    std::memcpy(p->added_mass, am, sizeof am);
    std::memcpy(p->Dl, dl, sizeof dl);
    std::memcpy(p->Dnl, dnl, sizeof dnl);
    std::memcpy(p->K, K, sizeof K);
    for (int i = 0; i < 21; i++) p->Q[i] = 0.001;
    for (int i = 0; i < 12; i++) p->R12[i] = r12[i / 3];
    p->vel_inject = 2.0;
    p->compensate_coef = 0.032546960744430276;
    p->rotor_constant = 0.026546960744430276;
    p->inject_bias_g = 0;
}

static void make_const(const brov_eskf_params& p, EskfConst& c) {
    c.dt = p.dt; c.mass = p.mass; c.mzg = p.mass * p.ZG; c.g = p.g; c.wb = p.mass * p.g - p.bouyancy; c.vel_inject = p.vel_inject;
    c.inv_cc = 1.0 / p.compensate_coef; c.inv_rc = 1.0 / p.rotor_constant;
    for (int i = 0; i < 3; i++) { c.am[i] = p.added_mass[i]; c.Dl[i] = p.Dl[i]; c.Dnl[i] = p.Dnl[i]; }
    for (int i = 0; i < 18; i++) c.K3[i] = p.K[i];
    for (int i = 0; i < 21; i++) c.Q[i] = p.Q[i];
    for (int i = 0; i < 12; i++) c.R12[i] = p.R12[i];
    c.inject = p.inject_bias_g != 0; c.pad = 0;
}

// pure host function behind brov_eskf_reset and brov_eskf_set_state_host: the quaternions of n states
static int check_states(const char* who, const double* x, int n) {
    for (int b = 0; b < n; b++) {
        const double* q = x + (size_t)b * 22 + 6;
        const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        if (!(std::fabs(std::sqrt(n2) - 1.0) <= 1e-6))
            return refuse(who, "the quaternion of state " + std::to_string(b) + " is not finite or not of unit length");
    }
    return BROV_OK;
}

extern "C" void brov_eskf_destroy(brov_eskf* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    e->mem.free_all();
    e->timer.destroy();
    delete e;
}

extern "C" int brov_eskf_reset(brov_eskf* e, const double* x0, const double* P0) {
    if (x0)
        if (int rc = check_states("brov_eskf_reset", x0, 1)) return rc;
    if (!e) return refuse("brov_eskf_reset", "null handle");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->last_stream));
    double xr[22] = {0};
    xr[6] = 1.0; xr[18] = -e->par.g;
    std::vector<double> hx((size_t)e->B * 22), hp((size_t)e->B * 441, 0.0);
    for (int b = 0; b < e->B; b++) {
        std::memcpy(&hx[(size_t)b * 22], x0 ? x0 : xr, sizeof xr);
        if (P0) std::memcpy(&hp[(size_t)b * 441], P0, 441 * sizeof(double));
    }
    HIPCHK(hipMemcpy(e->x, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->P, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice));
    e->first = true;
    return BROV_OK;
}

extern "C" int brov_eskf_create(brov_eskf** out, int device, int B, const brov_eskf_params* p) {
    if (!out) return refuse("brov_eskf_create", "null argument");
    *out = nullptr;
    if (B <= 0) return refuse("brov_eskf_create", "the batch must be positive");
    brov_eskf_params par;
    if (p) par = *p; else brov_eskf_default_params(&par);
    if (!(par.dt > 0.0) || !(par.gps_dt > 0.0)) return refuse("brov_eskf_create", "dt and gps_dt must be positive");
    for (int i = 0; i < 12; i++)
        if (!(par.R12[i] > 0.0)) return refuse("brov_eskf_create", "R12[" + std::to_string(i) + "] must be positive");
    if (!usable_device(device)) {
        g_eskf_err = "brov_eskf_create: no usable HIP device (the observer has no CPU path)";
        return BROV_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(device));
    brov_eskf* e = new brov_eskf();
    e->device = device; e->B = B; e->par = par;
    make_const(e->par, e->c);
    int rc = BROV_OK;
    auto al = [&](auto** q, size_t n) { return rc = e->mem.alloc(q, n, g_eskf_err); };
    const size_t nb = (size_t)B;
    if (al(&e->x, nb * 22) || al(&e->P, nb * 441) || al(&e->imu, nb * 6) || al(&e->gps_p, nb * 3) || al(&e->gps_v, nb * 3) || al(&e->qm, nb * 4) ||
        al(&e->thrust, nb * 6) || al(&e->xi, nb * 3) || al(&e->xw, nb * 3) || al(&e->mp, nb * 4) || al(&e->vprev, nb * 3) || al(&e->pprev, nb * 3) ||
        al(&e->status, nb) || al(&e->cdev, 1)) {
        g_eskf_err = "brov_eskf_create: " + g_eskf_err;
        brov_eskf_destroy(e);
        return rc;
    }
    bool good = hipMemcpy(e->cdev, &e->c, sizeof(EskfConst), hipMemcpyHostToDevice) == hipSuccess && e->timer.create() == hipSuccess;
    for (double* q : {e->gps_p, e->gps_v, e->xi, e->xw, e->vprev, e->pprev})
        good = good && hipMemset(q, 0, nb * 3 * sizeof(double)) == hipSuccess;
    good = good && hipMemset(e->imu, 0, nb * 6 * sizeof(double)) == hipSuccess && hipMemset(e->thrust, 0, nb * 6 * sizeof(double)) == hipSuccess &&
           hipMemset(e->qm, 0, nb * 4 * sizeof(double)) == hipSuccess && hipMemset(e->mp, 0, nb * 4 * sizeof(double)) == hipSuccess &&
           hipMemset(e->status, 0, nb * sizeof(int)) == hipSuccess;
    if (!good) {
        (void)hipGetLastError();
        g_eskf_err = "brov_eskf_create: device initialisation failed";
        brov_eskf_destroy(e);
        return BROV_ERR_HIP;
    }
    rc = brov_eskf_reset(e, nullptr, nullptr);
    if (rc) { brov_eskf_destroy(e); return rc; }
    *out = e;
    return BROV_OK;
}

extern "C" int brov_eskf_batch(const brov_eskf* e) { return e ? e->B : 0; }

extern "C" int brov_eskf_set_state_host(brov_eskf* e, const double* x, const double* P) {
    if (!e) return refuse("brov_eskf_set_state_host", "null handle");
    if (x)
        if (int rc = check_states("brov_eskf_set_state_host", x, e->B)) return rc;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->last_stream));
    if (x) HIPCHK(hipMemcpy(e->x, x, (size_t)e->B * 22 * sizeof(double), hipMemcpyHostToDevice));
    if (P) HIPCHK(hipMemcpy(e->P, P, (size_t)e->B * 441 * sizeof(double), hipMemcpyHostToDevice));
    e->first = true;
    return BROV_OK;
}

extern "C" int brov_eskf_get_state_host(brov_eskf* e, double* x, double* P) {
    if (!e) return refuse("brov_eskf_get_state_host", "null handle");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->last_stream));
    if (x) HIPCHK(hipMemcpy(x, e->x, (size_t)e->B * 22 * sizeof(double), hipMemcpyDeviceToHost));
    if (P) HIPCHK(hipMemcpy(P, e->P, (size_t)e->B * 441 * sizeof(double), hipMemcpyDeviceToHost));
    return BROV_OK;
}

static int launch_tick(brov_eskf* e, bool update, const double* imu, const double* gps_p, const double* gps_v, const double* qm, const double* thrust,
                       hipStream_t st) {
    EskfArgs a;
    a.c = e->cdev; a.B = e->B; a.x = e->x; a.P = e->P; a.imu = imu; a.gps_p = gps_p; a.gps_v = gps_v; a.qm = qm; a.thrust = thrust;
    a.xi = e->xi; a.xw = e->xw; a.mp = e->mp; a.status = e->status;
    HIPCHK(e->timer.start(st));
    const int blocks = (e->B + kEskfFilters - 1) / kEskfFilters;
    if (update) hipLaunchKernelGGL(eskf_tick_kernel<true>, dim3(blocks), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(eskf_tick_kernel<false>, dim3(blocks), dim3(64), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(e->timer.stop(st));
    e->last_stream = st;
    return BROV_OK;
}

extern "C" int brov_eskf_predict_device(brov_eskf* e, const double* imu, void* stream) {
    if (!e || !imu) return refuse("brov_eskf_predict_device", "null argument");
    HIPCHK(hipSetDevice(e->device));
    return launch_tick(e, false, imu, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int brov_eskf_predict_host(brov_eskf* e, const double* imu, void* stream) {
    if (!e || !imu) return refuse("brov_eskf_predict_host", "null argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(e->imu, imu, (size_t)e->B * 6 * sizeof(double), hipMemcpyHostToDevice, st));
    return launch_tick(e, false, e->imu, nullptr, nullptr, nullptr, nullptr, st);
}

extern "C" int brov_eskf_update_device(brov_eskf* e, const double* imu, const double* gps_p, const double* gps_v, const double* q_meas,
                                       const double* thrust, void* stream) {
    if (!e || !imu || !gps_p || !gps_v || !q_meas || !thrust) return refuse("brov_eskf_update_device", "null argument");
    HIPCHK(hipSetDevice(e->device));
    return launch_tick(e, true, imu, gps_p, gps_v, q_meas, thrust, (hipStream_t)stream);
}

extern "C" int brov_eskf_update_host(brov_eskf* e, const double* imu, const double* gps_p, const double* gps_v, const double* q_meas,
                                     const double* thrust, void* stream) {
    if (!e || !imu || !gps_p || !gps_v || !q_meas || !thrust) return refuse("brov_eskf_update_host", "null argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = (size_t)e->B * sizeof(double);
    HIPCHK(hipMemcpyAsync(e->imu, imu, nb * 6, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->gps_p, gps_p, nb * 3, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->gps_v, gps_v, nb * 3, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->qm, q_meas, nb * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->thrust, thrust, nb * 6, hipMemcpyHostToDevice, st));
    return launch_tick(e, true, e->imu, e->gps_p, e->gps_v, e->qm, e->thrust, st);
}

extern "C" int brov_eskf_get_outputs_host(brov_eskf* e, double* xi, double* xi_world, double* mpc_p, int* status) {
    if (!e) return refuse("brov_eskf_get_outputs_host", "null handle");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->last_stream));
    if (xi) HIPCHK(hipMemcpy(xi, e->xi, (size_t)e->B * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (xi_world) HIPCHK(hipMemcpy(xi_world, e->xw, (size_t)e->B * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (mpc_p) HIPCHK(hipMemcpy(mpc_p, e->mp, (size_t)e->B * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, e->status, (size_t)e->B * sizeof(int), hipMemcpyDeviceToHost));
    return BROV_OK;
}

extern "C" int brov_eskf_get_inputs_host(brov_eskf* e, double* imu, double* gps_p, double* gps_v, double* q_meas, double* thrust) {
    if (!e) return refuse("brov_eskf_get_inputs_host", "null handle");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->last_stream));
    const size_t nb = (size_t)e->B * sizeof(double);
    if (imu) HIPCHK(hipMemcpy(imu, e->imu, nb * 6, hipMemcpyDeviceToHost));
    if (gps_p) HIPCHK(hipMemcpy(gps_p, e->gps_p, nb * 3, hipMemcpyDeviceToHost));
    if (gps_v) HIPCHK(hipMemcpy(gps_v, e->gps_v, nb * 3, hipMemcpyDeviceToHost));
    if (q_meas) HIPCHK(hipMemcpy(q_meas, e->qm, nb * 4, hipMemcpyDeviceToHost));
    if (thrust) HIPCHK(hipMemcpy(thrust, e->thrust, nb * 6, hipMemcpyDeviceToHost));
    return BROV_OK;
}

extern "C" const double* brov_eskf_x_device(const brov_eskf* e) { return e ? e->x : nullptr; }
extern "C" const double* brov_eskf_P_device(const brov_eskf* e) { return e ? e->P : nullptr; }
extern "C" const double* brov_eskf_mpc_p_device(const brov_eskf* e) { return e ? e->mp : nullptr; }

extern "C" int brov_eskf_update_from_solver(brov_eskf* e, brov_solver* s, void* stream) {
    if (!e || !s || brov_batch(s) != e->B) return refuse("brov_eskf_update_from_solver", "batch sizes differ");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    if (brov_order_stream(s, stream) != BROV_OK) { g_eskf_err = "brov_eskf_update_from_solver: could not order behind the solver's last stream"; return BROV_ERR_HIP; }
    if (e->last_stream != st) HIPCHK(hipStreamSynchronize(e->last_stream));
    hipLaunchKernelGGL(eskf_inputs_from_solver_kernel, dim3((e->B + 255) / 256), dim3(256), 0, st, e->B, e->par.dt, e->par.gps_dt, e->par.g, 1.0 / kRotor,
                       e->first ? 1 : 0, solver_measured_state(s), solver_observer_results(s), e->vprev, e->pprev, e->imu, e->gps_p, e->gps_v, e->qm,
                       e->thrust);
    HIPCHK(hipGetLastError());
    e->first = false;
    return launch_tick(e, true, e->imu, e->gps_p, e->gps_v, e->qm, e->thrust, st);
}

extern "C" int brov_eskf_apply_to_solver(brov_eskf* e, brov_solver* s, void* stream) {
    if (!e || !s || brov_batch(s) != e->B) return refuse("brov_eskf_apply_to_solver", "batch sizes differ");
    HIPCHK(hipSetDevice(e->device));
    brov_opts o;
    if (brov_get_opts(s, &o) != BROV_OK) return refuse("brov_eskf_apply_to_solver", "the solver's options cannot be read");
    const int stages = o.N + 1;
    const long long n = (long long)e->B * stages;
    if (brov_order_stream(s, stream) != BROV_OK) { g_eskf_err = "brov_eskf_apply_to_solver: could not order behind the solver's last stream"; return BROV_ERR_HIP; }
    if (e->last_stream != (hipStream_t)stream) HIPCHK(hipStreamSynchronize(e->last_stream));
    hipLaunchKernelGGL(eskf_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, e->B, stages, (const double*)e->mp,
                       brov_params_device(s));
    HIPCHK(hipGetLastError());
    e->last_stream = (hipStream_t)stream;
    return BROV_OK;
}

extern "C" int brov_eskf_last_update_seconds(brov_eskf* e, double* seconds) {
    if (!e || !seconds || !e->timer.valid) return refuse("brov_eskf_last_update_seconds", "null argument, or no tick has been timed");
    HIPCHK(hipSetDevice(e->device));
    return e->timer.seconds(seconds, g_eskf_err);
}
