// eskf_kernel.hip -- batched error-state Kalman filter with IMU disturbance observer and its C ABI (include/bluerov2_nmpc_eskf.h, brov_eskf_*).
// B independent copies of the reference's bluerov2_states nodelet (src/Eskf.cpp: predict :97-158, update :197-306, inject :320-332;
// Dynamics.cpp; Config.cpp): nominal state [p | v | q | b_g | b_a | g_I | xi] (22), covariance over the 21 error states, whose last three are the
// body-frame disturbance force the "patty" DOB node and the consolidated controller's DOMPC mode take from /disturbance.  The formulas stand in
// the header; tests/eskf_exact.py restates them at 60 digits.
//
// One kernel body (eskf_tick_body.inc), in eskf_tick_kernel<UPDATE>: predict only, or predict followed by update; and in eskf_tick_masked_kernel:
// per filter the one or the other, by a flag (the filter at its sensors' rates, include/bluerov2_nmpc_imu.h).  Layout: one filter per 32 lanes (two per wave, one
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
#include "eskf_tick_body.inc"
}
// fix [B]: 0 the predict-only tick, else the update tick, per filter; bit for bit what the two kernels above give (see eskf_tick_body.inc)
__global__ __launch_bounds__(64, 2) void eskf_tick_masked_kernel(EskfArgs A, const int* __restrict__ fix) {
    constexpr bool UPDATE = true;
#define ESKF_TICK_MASKED
#include "eskf_tick_body.inc"
#undef ESKF_TICK_MASKED
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

// the filter's inputs from the solver's IMU/GPS stage (one lane per filter): the stage's last sample and its flags into the observer's own
// buffers -- what the tick reads and brov_eskf_get_inputs_host returns --, thrust as eskf_inputs_from_solver_kernel has it
__global__ void eskf_inputs_from_imu_kernel(int B, double inv_rc, const double* __restrict__ s_imu, const double* __restrict__ s_gp,
                                            const double* __restrict__ s_gv, const double* __restrict__ s_qm, const int32_t* __restrict__ s_fix,
                                            const brov_result* __restrict__ res, double* __restrict__ imu, double* __restrict__ gps_p,
                                            double* __restrict__ gps_v, double* __restrict__ qm, double* __restrict__ thrust, int* __restrict__ fix) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
#pragma unroll
    for (int k = 0; k < 6; k++) imu[(size_t)b * 6 + k] = s_imu[(size_t)b * 6 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) { gps_p[(size_t)b * 3 + k] = s_gp[(size_t)b * 3 + k]; gps_v[(size_t)b * 3 + k] = s_gv[(size_t)b * 3 + k]; }
#pragma unroll
    for (int k = 0; k < 4; k++) qm[(size_t)b * 4 + k] = s_qm[(size_t)b * 4 + k];
    fix[b] = s_fix[b];
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
    int* fix = nullptr;  // [B] the flags of the last masked tick that copied them (brov_imu_eskf_tick_host, brov_imu_eskf_tick_from_solver)
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
        al(&e->status, nb) || al(&e->fix, nb) || al(&e->cdev, 1)) {
        g_eskf_err = "brov_eskf_create: " + g_eskf_err;
        brov_eskf_destroy(e);
        return rc;
    }
    bool good = hipMemcpy(e->cdev, &e->c, sizeof(EskfConst), hipMemcpyHostToDevice) == hipSuccess && e->timer.create() == hipSuccess;
    for (double* q : {e->gps_p, e->gps_v, e->xi, e->xw, e->vprev, e->pprev})
        good = good && hipMemset(q, 0, nb * 3 * sizeof(double)) == hipSuccess;
    good = good && hipMemset(e->imu, 0, nb * 6 * sizeof(double)) == hipSuccess && hipMemset(e->thrust, 0, nb * 6 * sizeof(double)) == hipSuccess &&
           hipMemset(e->qm, 0, nb * 4 * sizeof(double)) == hipSuccess && hipMemset(e->mp, 0, nb * 4 * sizeof(double)) == hipSuccess &&
           hipMemset(e->status, 0, nb * sizeof(int)) == hipSuccess && hipMemset(e->fix, 0, nb * sizeof(int)) == hipSuccess;
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

// fix: null, the kernel `update` names for every filter; else [B] DEVICE, the masked kernel
static int launch_tick(brov_eskf* e, bool update, const double* imu, const double* gps_p, const double* gps_v, const double* qm, const double* thrust,
                       hipStream_t st, const int* fix = nullptr) {
    EskfArgs a;
    a.c = e->cdev; a.B = e->B; a.x = e->x; a.P = e->P; a.imu = imu; a.gps_p = gps_p; a.gps_v = gps_v; a.qm = qm; a.thrust = thrust;
    a.xi = e->xi; a.xw = e->xw; a.mp = e->mp; a.status = e->status;
    HIPCHK(e->timer.start(st));
    const int blocks = (e->B + kEskfFilters - 1) / kEskfFilters;
    if (fix) hipLaunchKernelGGL(eskf_tick_masked_kernel, dim3(blocks), dim3(64), 0, st, a, fix);
    else if (update) hipLaunchKernelGGL(eskf_tick_kernel<true>, dim3(blocks), dim3(64), 0, st, a);
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

extern "C" int brov_imu_eskf_tick_device(brov_eskf* e, const double* imu, const double* gps_p, const double* gps_v, const double* q_meas,
                                     const double* thrust, const int32_t* fix, void* stream) {
    if (!e || !imu || !gps_p || !gps_v || !q_meas || !thrust || !fix) return refuse("brov_imu_eskf_tick_device", "null argument");
    HIPCHK(hipSetDevice(e->device));
    return launch_tick(e, true, imu, gps_p, gps_v, q_meas, thrust, (hipStream_t)stream, fix);
}

extern "C" int brov_imu_eskf_tick_host(brov_eskf* e, const double* imu, const double* gps_p, const double* gps_v, const double* q_meas,
                                   const double* thrust, const int32_t* fix, void* stream) {
    if (!e || !imu || !gps_p || !gps_v || !q_meas || !thrust || !fix) return refuse("brov_imu_eskf_tick_host", "null argument");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = (size_t)e->B * sizeof(double);
    HIPCHK(hipMemcpyAsync(e->imu, imu, nb * 6, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->gps_p, gps_p, nb * 3, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->gps_v, gps_v, nb * 3, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->qm, q_meas, nb * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->thrust, thrust, nb * 6, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->fix, fix, (size_t)e->B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    return launch_tick(e, true, e->imu, e->gps_p, e->gps_v, e->qm, e->thrust, st, e->fix);
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
extern "C" const double* brov_imu_eskf_xi_world_device(const brov_eskf* e) { return e ? e->xw : nullptr; }

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

// the tick at the sensors' rates: the sample of the solver's IMU/GPS stage; predict only where no fix was due at its index, else the masked tick
extern "C" int brov_imu_eskf_tick_from_solver(brov_eskf* e, brov_solver* s, void* stream) {
    if (!e || !s || brov_batch(s) != e->B) return refuse("brov_imu_eskf_tick_from_solver", "batch sizes differ");
    const ImuView v = solver_imu_view(s);
    if (!v.on) return refuse("brov_imu_eskf_tick_from_solver", "the IMU stage of the solver is off (brov_imu_set_host)");
    if (v.h != e->par.dt) return refuse("brov_imu_eskf_tick_from_solver", "the filter's dt is not the step h the solver's IMU stage samples");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    if (brov_order_stream(s, stream) != BROV_OK) { g_eskf_err = "brov_imu_eskf_tick_from_solver: could not order behind the solver's last stream"; return BROV_ERR_HIP; }
    if (e->last_stream != st) HIPCHK(hipStreamSynchronize(e->last_stream));
    hipLaunchKernelGGL(eskf_inputs_from_imu_kernel, dim3((e->B + 255) / 256), dim3(256), 0, st, e->B, 1.0 / kRotor, v.imu, v.gps_p, v.gps_v, v.qm, v.fix,
                       solver_observer_results(s), e->imu, e->gps_p, e->gps_v, e->qm, e->thrust, e->fix);
    HIPCHK(hipGetLastError());
    if (!v.fix_due) return launch_tick(e, false, e->imu, nullptr, nullptr, nullptr, nullptr, st);
    return launch_tick(e, true, e->imu, e->gps_p, e->gps_v, e->qm, e->thrust, st, e->fix);
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
