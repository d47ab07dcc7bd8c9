// track_kernel.hip -- batched tracking statistics of closed loops and their C ABI (include/bluerov2_nmpc.h, brov_track_*): one 96-byte
// record per instance (squared position / yaw error sums and maxima against the trajectory table, input energy, counts of failed,
// saturated and non-finite ticks), fed from device logs [K][B][..] of K consecutive ticks, and a summary of the whole batch.
//
// track_accumulate_kernel: one lane per instance.  The record is loaded once, updated over the K ticks in tick order and stored once;
// per tick a lane reads 4 of the 12 state columns, the 4 inputs and the status (68 B; the shared reference row comes through the scalar
// cache).  No LDS, no cross-lane traffic: a streaming kernel.  Because the order within an instance is the tick order, the record does
// not depend on how a run is cut into calls.
//
// Bit-equality.  Maxima are compared exactly against the numpy restatement (tests/track_restatement.py), so the squares and their sums
// are plain IEEE * and + in the order written -- no contraction into FMAs (the pragma below; hipcc contracts across statements by
// default).  Finiteness is tested on the exponent bits: an ordering comparison is false for NaN on either side and would let one through.
//
// track_reduce_kernel + track_finish_kernel: the batch summary without floating-point atomics.  A fixed grid (a function of B only), every
// thread folds its instances in ascending order, a wavefront folds over its 64 lanes with shuffles, a block over its waves through LDS
// and writes ONE partial; a single thread then folds the partials in index order.  The same B gives the same order, so two calls
// return the same bytes.  The arg-max travels as a (value, index) pair; on equal values the lower index wins at every level.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "bluerov2_nmpc.h"

static_assert(sizeof(brov_track_stats) == 96, "brov_track_stats is a 96-byte record");
static_assert(sizeof(brov_track_summary) == 64, "brov_track_summary");

namespace brov {

constexpr int kTrackBlock = 256;
constexpr int kTrackWaves = kTrackBlock / 64;
constexpr int kTrackMaxPartials = 1024;

struct TrackArgs {
    int B, K, rows;
    long long line1;
    const double *x, *u;      // [K][B][12], [K][B][4]
    const int* status;        // [K][B] or null
    const double* ref;        // [rows][16]
    double lbu[4], ubu[4];
    brov_track_stats* rec;    // [B]
};

__device__ __forceinline__ bool track_finite(double v) { return (__double2hiint(v) & 0x7ff00000) != 0x7ff00000; }

__global__ __launch_bounds__(kTrackBlock) void track_accumulate_kernel(TrackArgs A) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= A.B) return;   // lane and block tails
    brov_track_stats r = A.rec[b];
    for (int j = 0; j < A.K; j++) {
        long long row = A.line1 + j;
        if (row > A.rows - 1) row = A.rows - 1;
        if (row < 0) row = 0;
        const double* __restrict__ yr = A.ref + (size_t)row * 16;
        const size_t jb = (size_t)j * A.B + b;
        const double* __restrict__ xs = A.x + jb * 12;
        const double* __restrict__ us = A.u + jb * 4;
        const double px = xs[0], py = xs[1], pz = xs[2], psi = xs[5];
        const double u0 = us[0], u1 = us[1], u2 = us[2], u3 = us[3];
        const int st = A.status ? A.status[jb] : 0;
        const int tick = r.ticks + r.nonfinite;   // numbered from the last reset
        if (st != 0) {
            r.failed++;
            if (r.first_failed < 0) r.first_failed = tick;
        }
        const bool fin = track_finite(px) && track_finite(py) && track_finite(pz) && track_finite(psi) && track_finite(u0) && track_finite(u1) &&
                         track_finite(u2) && track_finite(u3);
        if (!fin) {
            r.nonfinite++;
            continue;
        }
        const double dx = px - yr[0], dy = py - yr[1], dz = pz - yr[2], dpsi = psi - yr[5];
        const double e2 = (dx * dx + dy * dy) + dz * dz;
        const double ay = fabs(dpsi);
        r.sum_pos2 = r.sum_pos2 + e2;
        r.sum_yaw2 = r.sum_yaw2 + dpsi * dpsi;
        r.sum_u2[0] = r.sum_u2[0] + u0 * u0;
        r.sum_u2[1] = r.sum_u2[1] + u1 * u1;
        r.sum_u2[2] = r.sum_u2[2] + u2 * u2;
        r.sum_u2[3] = r.sum_u2[3] + u3 * u3;
        if (r.ticks == 0 || e2 > r.max_pos2) {
            r.max_pos2 = e2;
            r.worst_tick = tick;
        }
        if (ay > r.max_yaw) r.max_yaw = ay;
        const bool sat = u0 <= A.lbu[0] || u0 >= A.ubu[0] || u1 <= A.lbu[1] || u1 >= A.ubu[1] || u2 <= A.lbu[2] || u2 >= A.ubu[2] ||
                         u3 <= A.lbu[3] || u3 >= A.ubu[3];
        if (sat) r.saturated++;
        r.ticks++;
    }
    A.rec[b] = r;
}

// what the summary is made of; idx < 0: no instance with a counted tick yet
struct TrackPartial {
    double sp, sy, mx;
    long long ticks, failed, sat, nonf;
    int idx, finst;
};
static_assert(sizeof(TrackPartial) == 64, "TrackPartial");

__device__ __forceinline__ TrackPartial track_identity() {
    TrackPartial p;
    p.sp = 0.0; p.sy = 0.0; p.mx = 0.0;
    p.ticks = 0; p.failed = 0; p.sat = 0; p.nonf = 0;
    p.idx = -1; p.finst = 0;
    return p;
}
// a := a (+) b; the arg-max keeps the larger value, on equal values the lower index
__device__ __forceinline__ void track_fold(TrackPartial& a, const TrackPartial& b) {
    a.sp = a.sp + b.sp;
    a.sy = a.sy + b.sy;
    a.ticks += b.ticks; a.failed += b.failed; a.sat += b.sat; a.nonf += b.nonf;
    a.finst += b.finst;
    if (b.idx >= 0 && (a.idx < 0 || b.mx > a.mx || (b.mx == a.mx && b.idx < a.idx))) {
        a.mx = b.mx;
        a.idx = b.idx;
    }
}
__device__ __forceinline__ TrackPartial track_shfl_down(const TrackPartial& p, int off) {
    TrackPartial q;
    q.sp = __shfl_down(p.sp, off, 64);
    q.sy = __shfl_down(p.sy, off, 64);
    q.mx = __shfl_down(p.mx, off, 64);
    q.ticks = __shfl_down(p.ticks, off, 64);
    q.failed = __shfl_down(p.failed, off, 64);
    q.sat = __shfl_down(p.sat, off, 64);
    q.nonf = __shfl_down(p.nonf, off, 64);
    q.idx = __shfl_down(p.idx, off, 64);
    q.finst = __shfl_down(p.finst, off, 64);
    return q;
}

__global__ __launch_bounds__(kTrackBlock) void track_reduce_kernel(const brov_track_stats* __restrict__ rec, int B, TrackPartial* __restrict__ partial) {
    __shared__ TrackPartial wave_part[kTrackWaves];
    TrackPartial acc = track_identity();
    const int stride = gridDim.x * blockDim.x;
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += stride) {   // ascending: tails hold the identity
        const brov_track_stats* r = rec + b;
        TrackPartial p = track_identity();
        p.failed = r->failed; p.nonf = r->nonfinite;
        p.finst = r->failed > 0 ? 1 : 0;
        if (r->ticks > 0) {
            p.sp = r->sum_pos2; p.sy = r->sum_yaw2; p.mx = r->max_pos2;
            p.ticks = r->ticks; p.sat = r->saturated;
            p.idx = b;
        }
        track_fold(acc, p);
    }
    // the wavefront: after the step with offset `off` the lanes below `off` hold the fold of their residue class
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const TrackPartial q = track_shfl_down(acc, off);
        if ((int)(threadIdx.x & 63) + off < 64) track_fold(acc, q);
    }
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        TrackPartial t = wave_part[0];
        for (int w = 1; w < kTrackWaves; w++) track_fold(t, wave_part[w]);
        partial[blockIdx.x] = t;
    }
}

// the partials in index order, by one thread
__global__ void track_finish_kernel(const TrackPartial* __restrict__ partial, int n, TrackPartial* __restrict__ total) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    TrackPartial t = partial[0];
    for (int i = 1; i < n; i++) track_fold(t, partial[i]);
    *total = t;
}

}  // namespace brov

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
#include "host_common.hpp"   // (here, not at the top: the kernels above keep their line numbers in the compiler's resource report)

using namespace brov;

static thread_local std::string g_track_err;
#define HIPCHK(call) BROV_HIPCHK(g_track_err, call)

struct brov_track {
    int device = 0, B = 0;
    brov_track_params par{};
    brov_track_stats* rec = nullptr;       // [B]
    TrackPartial* partial = nullptr;       // [kTrackMaxPartials + 1]: one per block of the reduction, then the total
    void* stage = nullptr;                 // brov_track_accumulate_host: the caller's logs and table on the device (grows, never shrinks)
    size_t stage_bytes = 0;
    hipStream_t last_stream = nullptr;
    KernelTimer timer;                     // around the last accumulate kernel
    hipEvent_t ev_done = nullptr;          // behind the last enqueued work
    bool done_valid = false;
    DeviceAllocs mem;                      // rec, partial
};

extern "C" const char* brov_track_last_error(void) { return g_track_err.c_str(); }

extern "C" void brov_track_default_params(brov_track_params* p) {
    if (!p) return;
    brov_opts o;
    brov_default_opts(&o, 1, 0.05);
    for (int c = 0; c < BROV_NU; c++) { p->lbu[c] = o.lbu[c]; p->ubu[c] = o.ubu[c]; }
}

extern "C" void brov_track_destroy(brov_track* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipStreamSynchronize(t->last_stream);
    t->mem.free_all();
    if (t->stage) (void)hipFree(t->stage);
    t->timer.destroy();
    if (t->ev_done) (void)hipEventDestroy(t->ev_done);
    delete t;
}

extern "C" int brov_track_batch(const brov_track* t) { return t ? t->B : 0; }

// work on `st` behind whatever the tracker enqueued last, without a host wait
static int order_behind(brov_track* t, hipStream_t st) {
    if (t->done_valid && t->last_stream != st) HIPCHK(hipStreamWaitEvent(st, t->ev_done, 0));
    return BROV_OK;
}
static int enqueued_on(brov_track* t, hipStream_t st) {
    HIPCHK(hipEventRecord(t->ev_done, st));
    t->done_valid = true;
    t->last_stream = st;
    return BROV_OK;
}

extern "C" int brov_track_reset(brov_track* t) {
    if (!t) { g_track_err = "brov_track_reset: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(t->device));
    HIPCHK(hipStreamSynchronize(t->last_stream));
    brov_track_stats z;
    std::memset(&z, 0, sizeof z);
    z.first_failed = -1;
    z.worst_tick = -1;
    std::vector<brov_track_stats> h((size_t)t->B, z);
    HIPCHK(hipMemcpy(t->rec, h.data(), h.size() * sizeof(brov_track_stats), hipMemcpyHostToDevice));
    return BROV_OK;
}

extern "C" int brov_track_create(brov_track** out, int device, int B, const brov_track_params* p) {
    if (!out || B <= 0 || B > (1 << 28)) { g_track_err = "brov_track_create: bad arguments"; return BROV_ERR_ARG; }
    *out = nullptr;
    brov_track_params q;
    if (p) q = *p; else brov_track_default_params(&q);
    for (int c = 0; c < BROV_NU; c++)
        if (!(q.lbu[c] <= q.ubu[c])) { g_track_err = "brov_track_create: need lbu <= ubu"; return BROV_ERR_ARG; }
    if (!usable_device(device)) {
        g_track_err = "brov_track_create: no usable HIP device (the statistics have no CPU path)";
        return BROV_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(device));
    brov_track* t = new brov_track();
    t->device = device; t->B = B; t->par = q;
    int rc = t->mem.alloc(&t->rec, (size_t)B, g_track_err);
    if (rc == BROV_OK) rc = t->mem.alloc(&t->partial, (size_t)(kTrackMaxPartials + 1), g_track_err);
    if (rc != BROV_OK) {
        g_track_err = "brov_track_create: " + g_track_err;
        brov_track_destroy(t);
        return rc;
    }
    if (t->timer.create() != hipSuccess || hipEventCreateWithFlags(&t->ev_done, hipEventDisableTiming) != hipSuccess) {
        g_track_err = "brov_track_create: device initialisation failed";
        brov_track_destroy(t);
        return BROV_ERR_HIP;
    }
    if ((rc = brov_track_reset(t)) != BROV_OK) { brov_track_destroy(t); return rc; }
    *out = t;
    return BROV_OK;
}

namespace brov {
// one accumulate over DEVICE logs on `st`, saturation judged by the given bounds (brov_closed_loop_track passes the solver's)
int track_accumulate_on(brov_track* t, const double* x, const double* u, const int* status, int K, const double* ref, int rows, int line1,
                        const double* lbu, const double* ubu, hipStream_t st) {
    if (!t || !x || !u || !ref || K < 1 || rows < 1) {
        g_track_err = "brov_track_accumulate: bad argument (needs logs, K >= 1 and a table of at least one row)";
        return BROV_ERR_ARG;
    }
    HIPCHK(hipSetDevice(t->device));
    if (int rc = order_behind(t, st)) return rc;
    TrackArgs a;
    a.B = t->B; a.K = K; a.rows = rows; a.line1 = line1;
    a.x = x; a.u = u; a.status = status; a.ref = ref; a.rec = t->rec;
    for (int c = 0; c < 4; c++) { a.lbu[c] = lbu[c]; a.ubu[c] = ubu[c]; }
    HIPCHK(t->timer.start(st));
    hipLaunchKernelGGL(track_accumulate_kernel, dim3((t->B + kTrackBlock - 1) / kTrackBlock), dim3(kTrackBlock), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(t->timer.stop(st));
    return enqueued_on(t, st);
}
}  // namespace brov

extern "C" int brov_track_accumulate_device(brov_track* t, const double* x, const double* u, const int32_t* status, int K, const double* ref,
                                            int rows, int line1, void* stream) {
    if (!t) { g_track_err = "brov_track_accumulate_device: null argument"; return BROV_ERR_ARG; }
    return track_accumulate_on(t, x, u, status, K, ref, rows, line1, t->par.lbu, t->par.ubu, (hipStream_t)stream);
}

extern "C" int brov_track_accumulate_host(brov_track* t, const double* x, const double* u, const int32_t* status, int K, const double* ref,
                                          int rows, int line1) {
    if (!t || !x || !u || !ref || K < 1 || rows < 1) { g_track_err = "brov_track_accumulate_host: bad argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(t->device));
    HIPCHK(hipStreamSynchronize(t->last_stream));   // the staging buffer may still be read by the last accumulate
    const size_t n = (size_t)K * t->B;
    const size_t bx = n * 12 * sizeof(double), bu = n * 4 * sizeof(double), br = (size_t)rows * 16 * sizeof(double), bs = n * sizeof(int32_t);
    const size_t need = bx + bu + br + bs;          // doubles first: every block stays 8-byte aligned
    if (need > t->stage_bytes) {
        if (t->stage) { (void)hipFree(t->stage); t->stage = nullptr; t->stage_bytes = 0; }
        if (hipMalloc(&t->stage, need) != hipSuccess) {
            (void)hipGetLastError();
            g_track_err = "brov_track_accumulate_host: hipMalloc failed";
            return BROV_ERR_ALLOC;
        }
        t->stage_bytes = need;
    }
    char* base = (char*)t->stage;
    double *dx = (double*)base, *du = (double*)(base + bx), *dr = (double*)(base + bx + bu);
    int* ds = (int*)(base + bx + bu + br);
    HIPCHK(hipMemcpy(dx, x, bx, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(du, u, bu, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dr, ref, br, hipMemcpyHostToDevice));
    if (status) HIPCHK(hipMemcpy(ds, status, bs, hipMemcpyHostToDevice));
    return track_accumulate_on(t, dx, du, status ? ds : nullptr, K, dr, rows, line1, t->par.lbu, t->par.ubu, nullptr);
}

extern "C" int brov_track_get_stats_host(brov_track* t, brov_track_stats* stats) {
    if (!t || !stats) { g_track_err = "brov_track_get_stats_host: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(t->device));
    HIPCHK(hipStreamSynchronize(t->last_stream));
    HIPCHK(hipMemcpy(stats, t->rec, (size_t)t->B * sizeof(brov_track_stats), hipMemcpyDeviceToHost));
    return BROV_OK;
}

extern "C" int brov_track_get_summary_host(brov_track* t, brov_track_summary* out) {
    if (!t || !out) { g_track_err = "brov_track_get_summary_host: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(t->device));
    hipStream_t st = t->last_stream;
    int blocks = (t->B + kTrackBlock - 1) / kTrackBlock;
    if (blocks > kTrackMaxPartials) blocks = kTrackMaxPartials;
    hipLaunchKernelGGL(track_reduce_kernel, dim3(blocks), dim3(kTrackBlock), 0, st, (const brov_track_stats*)t->rec, t->B, t->partial);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(track_finish_kernel, dim3(1), dim3(64), 0, st, (const TrackPartial*)t->partial, blocks, t->partial + kTrackMaxPartials);
    HIPCHK(hipGetLastError());
    if (int rc = enqueued_on(t, st)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    TrackPartial p;
    HIPCHK(hipMemcpy(&p, t->partial + kTrackMaxPartials, sizeof p, hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->worst_instance = -1;
    out->ticks = p.ticks; out->failed = p.failed; out->saturated = p.sat; out->nonfinite = p.nonf;
    out->failed_instances = p.finst;
    if (p.ticks > 0) {
        out->rms_pos = std::sqrt(p.sp / (double)p.ticks);
        out->rms_yaw = std::sqrt(p.sy / (double)p.ticks);
        out->worst_max_pos2 = p.mx;
        out->worst_instance = p.idx;
    }
    return BROV_OK;
}

extern "C" int brov_track_last_seconds(brov_track* t, double* seconds) {
    if (!t || !seconds || !t->timer.valid) { g_track_err = "brov_track_last_seconds: no accumulate yet"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(t->device));
    return t->timer.seconds(seconds, g_track_err);
}
