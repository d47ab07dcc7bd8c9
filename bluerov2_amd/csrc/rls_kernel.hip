// rls_kernel.hip -- batched recursive least squares with a variable forgetting factor (RLS-FF), the parameter identification of the
// adaptive MPC node, and its C ABI (include/bluerov2_nmpc.h, brov_rls_*).  B independent copies of BLUEROV2_AMPC::RLSFF()
// (bluerov2_dobmpc/src/bluerov2_ampc.cpp:731-1046): four independent axes X, Y, Z, N, each with
//     regressor x = [acc, v, 1, v|v|], target y = the EKF's body-frame disturbance estimate esti_x(12 | 13 | 14 | 17),
//     e = y - x.theta,  two error windows (n_short = FF_n = 5, n_long = FF_d = 50, bluerov2_ampc.h:239-240),
//     F = var_short / var_long (two-pass mean / variance, oldest to newest),  lambda -/+ step with clamps at [lambda_min, lambda_max],
//     K = P x / (lambda + x.(P x)),  theta += K e,  P = (P - (K x^T) P) / lambda,
// the world-frame environmental disturbance wf_env (:1000-1005) and AMPC's hand-off to the NMPC parameters (:346-349, and the
// commented-out "fully adaptive" lines :355-378).
//
// One lane per (instance, axis): lane g = 4 b + a.  The state is structure-of-arrays in HBM, every array [component][4 B], so every
// load and store of a wavefront is one contiguous 512-byte run; the inputs [B][4] are already in lane order.  Each error window is a
// ring buffer [slot][4 B] with a count and a head per lane.  A streaming kernel: ~0.4 KFLOP against ~3.6 KB of HBM traffic per
// instance and tick (the long window is read twice), so no LDS and no MFMA.
//
// Bit-equality.  Once theta has converged the two window variances are at rounding-noise level and the forgetting factor follows
// their ratio through a threshold test: a last-bit difference flips decisions and the trajectories part.  So the update is plain IEEE
// + - * / in exactly the order above -- sums sequential in index order, no contraction into FMAs (the pragma below; hipcc contracts
// across statements by default), no reciprocal multiplies, no fast-math intrinsics -- and is bit-identical to a scalar restatement
// (tests/rlsff_restatement.py).  wf_env goes through sin / cos and is not.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "bluerov2_nmpc.h"

namespace brov {

// the EKF's last update event (ekf_kernel.hip): the on-device AMPC tick reads its estimate
int ekf_wait_last_update(const brov_ekf* e, hipStream_t st);

constexpr int kRlsMaxWin = 256;
constexpr int kRlsBlock = 256;

struct RlsArgs {
    int B, G;                      // G = 4 B lanes
    int ns, nl;                    // window lengths
    double thr, step, lmin, lmax, cc, rc;
    double *theta, *P, *lam, *F, *e;   // [4][G], [16][G], [G], [G], [G]
    double *ws, *wl;                   // [ns][G], [nl][G]
    int *cs, *hs, *cl, *hl;            // count / head of each window, [G]
    const double *y, *acc, *vel;       // [B][4] = [G]
    const double* rpy;                 // [B][3]
    double *wf, *mp;                   // [B][6], [B][4]
    int* status;                       // [B]
};

// push e onto a ring of n slots (count c, head h = next slot to write), then mean and variance of its c entries oldest to newest
__device__ __forceinline__ double rls_window_var(double* __restrict__ w, int* __restrict__ cnt, int* __restrict__ head, int n, int G,
                                                 int g, double err) {
    int h = head[g], c = cnt[g];
    w[(size_t)h * G + g] = err;
    h = h + 1 == n ? 0 : h + 1;
    c = c < n ? c + 1 : n;
    head[g] = h;
    cnt[g] = c;
    int first = h - c;
    if (first < 0) first += n;
    double sum = 0.0;
#pragma unroll 8
    for (int i = 0, k = first; i < c; i++) {
        sum = sum + w[(size_t)k * G + g];
        k = k + 1 == n ? 0 : k + 1;
    }
    const double mean = sum / (double)c;
    double var = 0.0;
#pragma unroll 8
    for (int i = 0, k = first; i < c; i++) {
        const double d = w[(size_t)k * G + g] - mean;
        var = var + d * d;
        k = k + 1 == n ? 0 : k + 1;
    }
    return var / (double)c;
}

__global__ __launch_bounds__(kRlsBlock) void rls_update_kernel(RlsArgs A) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.G) return;   // G and the block are multiples of 4: the four lanes of an instance are live together
    const int G = A.G, b = g >> 2, a = g & 3;
    double th[4], P[16];
#pragma unroll
    for (int i = 0; i < 4; i++) th[i] = A.theta[(size_t)i * G + g];
#pragma unroll
    for (int i = 0; i < 16; i++) P[i] = A.P[(size_t)i * G + g];
    double lam = A.lam[g];
    const double v = A.vel[g];
    const double x[4] = {A.acc[g], v, 1.0, v * fabs(v)};
    // prediction error with the old theta
    double xt = x[0] * th[0];
    xt = xt + x[1] * th[1];
    xt = xt + x[2] * th[2];
    xt = xt + x[3] * th[3];
    const double err = A.y[g] - xt;
    // F statistic of the two windows, forgetting factor
    const double vs = rls_window_var(A.ws, A.cs, A.hs, A.ns, G, g, err);
    const double vl = rls_window_var(A.wl, A.cl, A.hl, A.nl, G, g, err);
    const double F = vs / vl;
    if (F > A.thr) {
        const double dn = lam - A.step;
        lam = dn >= A.lmin ? dn : A.lmin;
    } else {
        const double up = lam + A.step;
        lam = up <= A.lmax ? up : A.lmax;
    }
    // gain, parameters, covariance
    double Px[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double s = P[i * 4] * x[0];
        s = s + P[i * 4 + 1] * x[1];
        s = s + P[i * 4 + 2] * x[2];
        s = s + P[i * 4 + 3] * x[3];
        Px[i] = s;
    }
    double xPx = x[0] * Px[0];
    xPx = xPx + x[1] * Px[1];
    xPx = xPx + x[2] * Px[2];
    xPx = xPx + x[3] * Px[3];
    const double den = lam + xPx;
    double K[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        K[i] = Px[i] / den;
        th[i] = th[i] + K[i] * err;
    }
    double Pn[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double M[4];
#pragma unroll
        for (int j = 0; j < 4; j++) M[j] = K[i] * x[j];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double s = M[0] * P[j];
            s = s + M[1] * P[4 + j];
            s = s + M[2] * P[8 + j];
            s = s + M[3] * P[12 + j];
            Pn[i * 4 + j] = (P[i * 4 + j] - s) / lam;
        }
    }
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        A.theta[(size_t)i * G + g] = th[i];
        fin = fin && fabs(th[i]) <= 1.7976931348623157e308;
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        A.P[(size_t)i * G + g] = Pn[i];
        fin = fin && fabs(Pn[i]) <= 1.7976931348623157e308;
    }
    A.lam[g] = lam;
    A.F[g] = F;
    A.e[g] = err;
    A.mp[g] = th[2] / (a < 2 ? A.cc : A.rc);   // bluerov2_ampc.cpp:346-349
    // per instance: status over the four axes, wf_env from theta(2) of all four (:1000-1005, rows 4-6 as written there)
    int bad = fin ? 0 : 1;
    bad |= __shfl_xor(bad, 1, 4);
    bad |= __shfl_xor(bad, 2, 4);
    const double tY = __shfl(th[2], 1, 4), tZ = __shfl(th[2], 2, 4), tN = __shfl(th[2], 3, 4);
    if (a != 0) return;
    const double tX = th[2];
    const double phi = A.rpy[(size_t)b * 3], the = A.rpy[(size_t)b * 3 + 1], psi = A.rpy[(size_t)b * 3 + 2];
    const double cf = cos(phi), sf = sin(phi), ct = cos(the), st = sin(the), cp = cos(psi), sp = sin(psi);
    double* wf = A.wf + (size_t)b * 6;
    wf[0] = (cp * ct) * tX + (-sp * cf + cp * st * sf) * tY + (sp * sf + cp * cf * st) * tZ;
    wf[1] = (sp * ct) * tX + (cp * cf + sf * st * sp) * tY + (-cp * sf + st * sp * cf) * tZ;
    wf[2] = (-st) * tX + (ct * sf) * tY + (ct * cf) * tZ;
    wf[3] = cf * st / ct * tN;
    wf[4] = (sf) * tN;
    wf[5] = (cf / ct) * tN;
    A.status[b] = bad ? 2 : 0;
}

// measurement assembly of the on-device AMPC tick: v = the plant's body velocities u, v, w, r (solver x0[6, 7, 8, 11]),
// acc = (v - v_prev) / dt (pose_cb, bluerov2_ampc.cpp:163-168), y = the EKF's estimate x[12, 13, 14, 17], rpy = x0[3..5]
__global__ void rls_inputs_kernel(int G, double dt, const double* __restrict__ x0, const double* __restrict__ xe, double* __restrict__ vprev,
                                  double* __restrict__ y, double* __restrict__ acc, double* __restrict__ vel, double* __restrict__ rpy) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int b = g >> 2, a = g & 3;
    const double v = x0[(size_t)b * 12 + (a < 3 ? 6 + a : 11)];
    acc[g] = (v - vprev[g]) / dt;
    vprev[g] = v;
    vel[g] = v;
    y[g] = xe[(size_t)b * 18 + (a < 3 ? 12 + a : 17)];
    if (a < 3) rpy[(size_t)b * 3 + a] = x0[(size_t)b * 12 + 3 + a];
}

// AMPC's hand-off (bluerov2_ampc.cpp:346-349) to every stage of instance b; model != 0 also the commented-out lines :355-378
__global__ void rls_apply_kernel(int B, int stages, int model, double cc, double rc, const double* __restrict__ theta, double* __restrict__ par) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= B * stages) return;
    const int b = k / stages, G = 4 * B;
    double* p = par + (size_t)k * 16;
    const double* t2 = theta + (size_t)2 * G + (size_t)b * 4;
    p[0] = t2[0] / cc;
    p[1] = t2[1] / cc;
    p[2] = t2[2] / rc;
    p[3] = t2[3] / rc;
    if (model) {
#pragma unroll
        for (int a = 0; a < 4; a++) {
            p[4 + a] = theta[(size_t)b * 4 + a];
            p[8 + a] = theta[(size_t)G + (size_t)b * 4 + a];
            p[12 + a] = theta[(size_t)3 * G + (size_t)b * 4 + a];
        }
    }
}

}  // namespace brov

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
#include "host_common.hpp"   // (here, not at the top: the kernels above keep their line numbers in the compiler's resource report)

using namespace brov;

static thread_local std::string g_rls_err;
#define HIPCHK(call) BROV_HIPCHK(g_rls_err, call)

struct brov_rls {
    int device = 0, B = 0, G = 0;
    brov_rls_params par{};
    double *theta = nullptr, *P = nullptr, *lam = nullptr, *F = nullptr, *e = nullptr, *ws = nullptr, *wl = nullptr;
    int *cs = nullptr, *hs = nullptr, *cl = nullptr, *hl = nullptr, *status = nullptr;
    double *y = nullptr, *acc = nullptr, *vel = nullptr, *rpy = nullptr, *vprev = nullptr, *wf = nullptr, *mp = nullptr;
    hipStream_t last_stream = nullptr, upd_stream = nullptr;
    KernelTimer timer;   // around the last update kernel
    DeviceAllocs mem;
};

extern "C" const char* brov_rls_last_error(void) { return g_rls_err.c_str(); }

extern "C" void brov_rls_default_params(brov_rls_params* p) {
    // bluerov2_ampc.h:171-180 (dt, compensate_coef, rotor_constant), :239-240 (FF_n, FF_d); bluerov2_ampc.cpp:735 (threshold) and the
    // lambda rule of :776-793; lambda_X..N = 0.9 and P = I at start-up
    std::memset(p, 0, sizeof(*p));
    p->n_short = 5;
    p->n_long = 50;
    p->threshold = 0.8;
    p->lambda_step = 0.01;
    p->lambda_min = 0.5;
    p->lambda_max = 1.0;
    p->lambda0 = 0.9;
    p->p0 = 1.0;
    p->dt = 0.05;
    p->compensate_coef = 0.032546960744430276;
    p->rotor_constant = 0.026546960744430276;
}

extern "C" void brov_rls_destroy(brov_rls* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    if (r->last_stream) (void)hipStreamSynchronize(r->last_stream);
    r->mem.free_all();
    r->timer.destroy();
    delete r;
}

extern "C" int brov_rls_batch(const brov_rls* r) { return r ? r->B : 0; }

// windows emptied; every pointer is written in full before it is next read
static int empty_windows(brov_rls* r) {
    const size_t n = (size_t)r->G * sizeof(int);
    HIPCHK(hipMemset(r->cs, 0, n));
    HIPCHK(hipMemset(r->hs, 0, n));
    HIPCHK(hipMemset(r->cl, 0, n));
    HIPCHK(hipMemset(r->hl, 0, n));
    return BROV_OK;
}

static int sync_last(brov_rls* r) {
    HIPCHK(hipStreamSynchronize(r->last_stream));
    return BROV_OK;
}

// HOST theta [B][4 axes][4], P [B][4][4][4], lambda [B][4]  <->  DEVICE [component][4 B]
static int upload_state(brov_rls* r, const double* th, const double* P, const double* lam) {
    const size_t G = r->G;
    if (th) {
        std::vector<double> h(4 * G);
        for (size_t g = 0; g < G; g++)
            for (int i = 0; i < 4; i++) h[i * G + g] = th[g * 4 + i];
        HIPCHK(hipMemcpy(r->theta, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (P) {
        std::vector<double> h(16 * G);
        for (size_t g = 0; g < G; g++)
            for (int i = 0; i < 16; i++) h[i * G + g] = P[g * 16 + i];
        HIPCHK(hipMemcpy(r->P, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (lam) HIPCHK(hipMemcpy(r->lam, lam, G * sizeof(double), hipMemcpyHostToDevice));
    return BROV_OK;
}

extern "C" int brov_rls_reset(brov_rls* r) {
    if (!r) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(r->device));
    if (int rc = sync_last(r)) return rc;
    const size_t G = r->G;
    std::vector<double> th(4 * G, 0.0), P(16 * G, 0.0), lam(G, r->par.lambda0);
    for (size_t g = 0; g < G; g++)
        for (int i = 0; i < 4; i++) P[g * 16 + i * 5] = r->par.p0;
    if (int rc = upload_state(r, th.data(), P.data(), lam.data())) return rc;
    HIPCHK(hipMemset(r->vprev, 0, G * sizeof(double)));
    HIPCHK(hipMemset(r->F, 0, G * sizeof(double)));
    HIPCHK(hipMemset(r->e, 0, G * sizeof(double)));
    HIPCHK(hipMemset(r->mp, 0, G * sizeof(double)));
    HIPCHK(hipMemset(r->wf, 0, (size_t)r->B * 6 * sizeof(double)));
    HIPCHK(hipMemset(r->status, 0, (size_t)r->B * sizeof(int)));
    return empty_windows(r);
}

extern "C" int brov_rls_create(brov_rls** out, int device, int B, const brov_rls_params* p) {
    if (!out || B <= 0 || B > (1 << 28)) { g_rls_err = "brov_rls_create: bad arguments"; return BROV_ERR_ARG; }
    *out = nullptr;
    brov_rls_params q;
    if (p) q = *p; else brov_rls_default_params(&q);
    if (q.n_short < 1 || q.n_short > kRlsMaxWin || q.n_long < 1 || q.n_long > kRlsMaxWin) {
        g_rls_err = "brov_rls_create: window lengths must lie in [1, 256]";
        return BROV_ERR_ARG;
    }
    if (!(0.0 < q.lambda_min && q.lambda_min <= q.lambda0 && q.lambda0 <= q.lambda_max) || !(q.dt > 0.0)) {
        g_rls_err = "brov_rls_create: need 0 < lambda_min <= lambda0 <= lambda_max and dt > 0";
        return BROV_ERR_ARG;
    }
    if (!usable_device(device)) {
        g_rls_err = "brov_rls_create: no usable HIP device (the estimator has no CPU path)";
        return BROV_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(device));
    brov_rls* r = new brov_rls();
    r->device = device; r->B = B; r->G = 4 * B; r->par = q;
    const size_t G = r->G;
    int rc = BROV_OK;
    auto al = [&](auto** p, size_t n) { return rc = r->mem.alloc(p, n, g_rls_err); };
    if (al(&r->theta, 4 * G) || al(&r->P, 16 * G) || al(&r->lam, G) || al(&r->F, G) || al(&r->e, G) || al(&r->ws, (size_t)q.n_short * G) ||
        al(&r->wl, (size_t)q.n_long * G) || al(&r->cs, G) || al(&r->hs, G) || al(&r->cl, G) || al(&r->hl, G) || al(&r->status, (size_t)B) ||
        al(&r->y, G) || al(&r->acc, G) || al(&r->vel, G) || al(&r->rpy, (size_t)B * 3) || al(&r->vprev, G) || al(&r->wf, (size_t)B * 6) ||
        al(&r->mp, G)) {
        g_rls_err = "brov_rls_create: " + g_rls_err;
        brov_rls_destroy(r);
        return rc;
    }
    if (r->timer.create() != hipSuccess) {
        g_rls_err = "brov_rls_create: device initialisation failed";
        brov_rls_destroy(r);
        return BROV_ERR_HIP;
    }
    rc = brov_rls_reset(r);
    if (rc) { brov_rls_destroy(r); return rc; }
    *out = r;
    return BROV_OK;
}

extern "C" int brov_rls_set_state_host(brov_rls* r, const double* theta, const double* P, const double* lambda) {
    if (!r) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(r->device));
    if (int rc = sync_last(r)) return rc;
    if (int rc = upload_state(r, theta, P, lambda)) return rc;
    return empty_windows(r);
}

extern "C" int brov_rls_get_state_host(brov_rls* r, double* theta, double* P, double* lambda, double* F, double* e) {
    if (!r) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(r->device));
    if (int rc = sync_last(r)) return rc;
    const size_t G = r->G;
    if (theta) {
        std::vector<double> h(4 * G);
        HIPCHK(hipMemcpy(h.data(), r->theta, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t g = 0; g < G; g++)
            for (int i = 0; i < 4; i++) theta[g * 4 + i] = h[i * G + g];
    }
    if (P) {
        std::vector<double> h(16 * G);
        HIPCHK(hipMemcpy(h.data(), r->P, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t g = 0; g < G; g++)
            for (int i = 0; i < 16; i++) P[g * 16 + i] = h[i * G + g];
    }
    if (lambda) HIPCHK(hipMemcpy(lambda, r->lam, G * sizeof(double), hipMemcpyDeviceToHost));
    if (F) HIPCHK(hipMemcpy(F, r->F, G * sizeof(double), hipMemcpyDeviceToHost));
    if (e) HIPCHK(hipMemcpy(e, r->e, G * sizeof(double), hipMemcpyDeviceToHost));
    return BROV_OK;
}

static int launch_update(brov_rls* r, const double* y, const double* acc, const double* vel, const double* rpy, hipStream_t st) {
    RlsArgs a;
    a.B = r->B; a.G = r->G; a.ns = r->par.n_short; a.nl = r->par.n_long;
    a.thr = r->par.threshold; a.step = r->par.lambda_step; a.lmin = r->par.lambda_min; a.lmax = r->par.lambda_max;
    a.cc = r->par.compensate_coef; a.rc = r->par.rotor_constant;
    a.theta = r->theta; a.P = r->P; a.lam = r->lam; a.F = r->F; a.e = r->e; a.ws = r->ws; a.wl = r->wl;
    a.cs = r->cs; a.hs = r->hs; a.cl = r->cl; a.hl = r->hl;
    a.y = y; a.acc = acc; a.vel = vel; a.rpy = rpy; a.wf = r->wf; a.mp = r->mp; a.status = r->status;
    HIPCHK(r->timer.start(st));
    hipLaunchKernelGGL(rls_update_kernel, dim3((r->G + kRlsBlock - 1) / kRlsBlock), dim3(kRlsBlock), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(r->timer.stop(st));
    r->last_stream = r->upd_stream = st;
    return BROV_OK;
}

extern "C" int brov_rls_update_device(brov_rls* r, const double* y, const double* acc, const double* vel, const double* rpy, void* stream) {
    if (!r || !y || !acc || !vel || !rpy) { g_rls_err = "brov_rls_update_device: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(r->device));
    return launch_update(r, y, acc, vel, rpy, (hipStream_t)stream);
}

extern "C" int brov_rls_update_host(brov_rls* r, const double* y, const double* acc, const double* vel, const double* rpy, void* stream) {
    if (!r || !y || !acc || !vel || !rpy) { g_rls_err = "brov_rls_update_host: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(r->device));
    hipStream_t st = (hipStream_t)stream;
    if (r->last_stream != st) if (int rc = sync_last(r)) return rc;   // the input buffers may still be read by the last update
    const size_t G = r->G;
    HIPCHK(hipMemcpyAsync(r->y, y, G * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r->acc, acc, G * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r->vel, vel, G * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r->rpy, rpy, (size_t)r->B * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    return launch_update(r, r->y, r->acc, r->vel, r->rpy, st);
}

extern "C" int brov_rls_update_from_ekf(brov_rls* r, const brov_ekf* ekf, brov_solver* s, void* stream) {
    if (!r || !ekf || !s || brov_batch(s) != r->B || brov_ekf_batch(ekf) != r->B) {
        g_rls_err = "brov_rls_update_from_ekf: batch sizes differ";
        return BROV_ERR_ARG;
    }
    HIPCHK(hipSetDevice(r->device));
    hipStream_t st = (hipStream_t)stream;
    if (brov_order_stream(s, stream) != BROV_OK) { g_rls_err = "brov_rls_update_from_ekf: could not order behind the solver's last stream"; return BROV_ERR_HIP; }
    if (ekf_wait_last_update(ekf, st) != BROV_OK) { g_rls_err = "brov_rls_update_from_ekf: could not order behind the EKF's last update"; return BROV_ERR_HIP; }
    if (r->last_stream != st) if (int rc = sync_last(r)) return rc;
    hipLaunchKernelGGL(rls_inputs_kernel, dim3((r->G + kRlsBlock - 1) / kRlsBlock), dim3(kRlsBlock), 0, st, r->G, r->par.dt,
                       solver_measured_state(s), brov_ekf_x_device(ekf), r->vprev, r->y, r->acc, r->vel, r->rpy);
    HIPCHK(hipGetLastError());
    return launch_update(r, r->y, r->acc, r->vel, r->rpy, st);
}

extern "C" int brov_rls_apply_to_solver(brov_rls* r, brov_solver* s, int mode, void* stream) {
    if (!r || !s || brov_batch(s) != r->B) { g_rls_err = "brov_rls_apply_to_solver: batch sizes differ"; return BROV_ERR_ARG; }
    if (mode != BROV_RLS_APPLY_DISTURBANCE && mode != BROV_RLS_APPLY_MODEL) { g_rls_err = "brov_rls_apply_to_solver: unknown mode"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(r->device));
    brov_opts o;
    if (brov_get_opts(s, &o) != BROV_OK) return BROV_ERR_ARG;
    const int stages = o.N + 1;
    const long long n = (long long)r->B * stages;
    hipStream_t st = (hipStream_t)stream;
    if (brov_order_stream(s, stream) != BROV_OK) { g_rls_err = "brov_rls_apply_to_solver: could not order behind the solver's last stream"; return BROV_ERR_HIP; }
    if (r->timer.valid && r->upd_stream != st) HIPCHK(hipStreamWaitEvent(st, r->timer.stop_event(), 0));
    hipLaunchKernelGGL(rls_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, r->B, stages, mode,
                       r->par.compensate_coef, r->par.rotor_constant, (const double*)r->theta, brov_params_device(s));
    HIPCHK(hipGetLastError());
    r->last_stream = st;
    return BROV_OK;
}

extern "C" int brov_rls_get_outputs_host(brov_rls* r, double* mpc_p, double* wf_env, int* status) {
    if (!r) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(r->device));
    if (int rc = sync_last(r)) return rc;
    if (mpc_p) HIPCHK(hipMemcpy(mpc_p, r->mp, (size_t)r->G * sizeof(double), hipMemcpyDeviceToHost));
    if (wf_env) HIPCHK(hipMemcpy(wf_env, r->wf, (size_t)r->B * 6 * sizeof(double), hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, r->status, (size_t)r->B * sizeof(int), hipMemcpyDeviceToHost));
    return BROV_OK;
}

extern "C" const double* brov_rls_theta_device(const brov_rls* r) { return r ? r->theta : nullptr; }

extern "C" int brov_rls_last_update_seconds(brov_rls* r, double* seconds) {
    if (!r || !seconds || !r->timer.valid) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(r->device));
    return r->timer.seconds(seconds, g_rls_err);
}
