// host_common.hpp -- the host-side scaffolding every device object of the C ABI is built from (brov_solver, brov_ekf, brov_rls, brov_track,
// brov_group): the HIP error check, the "is this device usable" test of the create calls, an owner of device allocations, a two-event kernel
// timer, the call context and the common part of the plant's stages, a scoped temporary device buffer, the logs of a closed loop.  Host code
// only, header only.  Each component keeps its OWN thread-local error string and brov_*_last_error(): a failing observer call must not
// overwrite brov_last_error(), so what reports here takes the string to write.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <functional>
#include <string>
#include <vector>

#include "../../include/bluerov2_nmpc.h"

namespace brov {

// ---- the HIP check ----------------------------------------------------------------------------------------------------------------
inline int hip_code(hipError_t e) {
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver) ? BROV_ERR_NO_DEVICE : BROV_ERR_HIP;
}
// `call` failed with `e`: its text into `err`, the code to return.  The error is reported here: it is not left behind as the thread's "last
// error" for an unrelated later call.
inline int hip_failed(std::string& err, const char* call, hipError_t e) {
    err = std::string(call) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    return hip_code(e);
}
// returns from the enclosing function when `call` fails; a component aliases it once: #define HIPCHK(call) BROV_HIPCHK(g_err, call)
#define BROV_HIPCHK(err, call)                                             \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) return ::brov::hip_failed(err, #call, e_);   \
    } while (0)

// ---- create calls: is `device` one this process can use?  Asked before anything is allocated; a refusal leaves no sticky error behind --------
inline bool usable_device(int device) {
    int ndev = 0;
    const bool ok = hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev;
    if (!ok) (void)hipGetLastError();
    return ok;
}

// ---- the device allocations an object makes once and keeps until it is destroyed (buffers that are replaced or grown during the object's
// life stay with the object) ---------------------------------------------------------------------------------------------------------------
struct DeviceAllocs {
    std::vector<void*> ptrs;
    size_t bytes = 0;
    template <typename T>
    int alloc(T** p, size_t n, std::string& err) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, n * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            err = "hipMalloc of " + std::to_string(n * sizeof(T)) + " bytes: " + hipGetErrorString(e);
            return BROV_ERR_ALLOC;
        }
        ptrs.push_back(q);
        bytes += n * sizeof(T);
        *p = (T*)q;
        return BROV_OK;
    }
    void free_all() {
        for (void* q : ptrs) (void)hipFree(q);
        ptrs.clear();
        bytes = 0;
    }
};

// ---- two events around the last launch of a kernel: its duration, and "that kernel has ended" for work on another stream ---------------------
struct KernelTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool valid = false;   // a launch has been timed: stop_event() and seconds() mean something
    hipError_t create() {
        const hipError_t e = hipEventCreate(&ev[0]);
        return e != hipSuccess ? e : hipEventCreate(&ev[1]);
    }
    void destroy() {
        for (hipEvent_t& e : ev)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
        valid = false;
    }
    hipError_t start(hipStream_t st) { return hipEventRecord(ev[0], st); }
    hipError_t stop(hipStream_t st) {
        const hipError_t e = hipEventRecord(ev[1], st);
        if (e == hipSuccess) valid = true;
        return e;
    }
    hipEvent_t stop_event() const { return ev[1]; }
    // waits for the timed launch to end; the caller has checked `valid`
    int seconds(double* out, std::string& err) {
        BROV_HIPCHK(err, hipEventSynchronize(ev[1]));
        float ms = 0.f;
        BROV_HIPCHK(err, hipEventElapsedTime(&ms, ev[0], ev[1]));
        *out = ms * 1e-3;
        return BROV_OK;
    }
};

// ---- what an entry point hands to the host side of a plant stage (wrench_source.hpp, thruster_source.hpp, sensor_source.hpp) with its own
// arguments.  Built per call in the calling thread by the owner's one helper and never stored: the error string is thread-local.  A method
// checks its arguments first and calls wait() once they have passed: a refused call waits for nothing and changes nothing.
struct CallCtx {
    std::function<int()> wait;   // the owner's: it selects the device, waits on the host for what may still use the buffers and returns a code
    DeviceAllocs& mem;           // the owner's allocations, which the stage's buffers come from
    std::string& err;            // the owner's error string ...
    const char* who;             // ... and the public name this call reports under
    int refuse(const char* why) const { err = std::string(who) + ": " + why; return BROV_ERR_ARG; }
};

// ---- what the two switchable stages of a solver's plant (ThrusterSource, SensorSource) have in common --------------------------------------
struct PlantStage {
    bool on = false;               // the stage is in force (off: everything as it always was)
    bool configured = false;       // the buffers hold a configuration (the last *_set_host's, or the defaults)
    size_t B = 0;                  // instances, set by the owner at create
    KernelTimer timer;             // around the last launch of the stage's kernel
    void destroy() { timer.destroy(); }
    int set_off() { on = false; return BROV_OK; }
    int last_seconds(double* seconds, const char* nothing_timed, const CallCtx& c) {
        if (!seconds || !timer.valid) return c.refuse(seconds ? nothing_timed : "null argument");
        return timer.seconds(seconds, c.err);
    }
    // one buffer of the stage on first use: from the owner's allocations, zeroed before the stage sees it (and, ahead of the first, the timer)
    template <typename T>
    int buffer(T** p, size_t n, const CallCtx& c) {
        T* q = nullptr;
        if (*p) return BROV_OK;
        if (!timer.ev[0]) BROV_HIPCHK(c.err, timer.create());
        if (int rc = c.mem.alloc(&q, n, c.err)) return rc;
        BROV_HIPCHK(c.err, hipMemset(q, 0, n * sizeof(T)));
        *p = q;
        return BROV_OK;
    }
};

// ---- what a component that is laid over a solver (brov_fleet) asks of it beyond the public accessors, without the side effects of the
// public hand-outs (brov_params_device marks the plant's copy of the parameters stale); filled by nmpc_api.hip -------------------------------
struct SolverView {
    int device = 0;
    const double* par = nullptr;          // [B][N+1][16] model parameters in force
    bool cand_set = false;                // candidate shape parameters are resident (brov_set_candidate_params_host)
    hipStream_t last_stream = nullptr;    // where the solver enqueued last: the stream its closed loops run on
};
SolverView solver_view(const brov_solver* s);
// [B][12] what the controller knows of the state: the measured state while the solver's sensor stage is on (brov_sensor_*), else the plant's
// own state, brov_x0_device(); read by the observer's and the estimator's *_from_solver / *_from_ekf updates
const double* solver_measured_state(const brov_solver* s);
// [B] the records whose thrusts brov_ekf_update_from_solver feeds the observer: the commanded ones, brov_results_device(), unless the solver's
// delay stage is on with observer_applied set (brov_delay_set_host): then what the last plant step was given; the rotor stage with its
// observer_applied set (brov_rotor_set_host) comes first: its applied records, the lagged ones;
// the thrust-curve stage with its flag set (brov_curve_set_host) comes ahead of both: the delivered forces
const brov_result* solver_observer_results(const brov_solver* s);
// the solver's IMU/GPS stage (brov_imu_*) as brov_imu_eskf_tick_from_solver reads it: whether it is on, the step h it samples, whether a fix was due
// at its last sample (else every flag is 0), and the DEVICE sample: imu [B][6], gps_p [B][3], gps_v [B][3], q_meas [B][4], fix [B]
struct ImuView {
    bool on = false, fix_due = false;
    double h = 0.0;
    const double *imu = nullptr, *gps_p = nullptr, *gps_v = nullptr, *qm = nullptr;
    const int32_t* fix = nullptr;
};
ImuView solver_imu_view(const brov_solver* s);

// ---- a device buffer that lives as long as a scope: freed on every way out, unless release() hands it on ---------------------------------
template <typename T>
struct ScopedDeviceBuffer {
    T* p = nullptr;
    ScopedDeviceBuffer() = default;
    ScopedDeviceBuffer(const ScopedDeviceBuffer&) = delete;
    ScopedDeviceBuffer& operator=(const ScopedDeviceBuffer&) = delete;
    ~ScopedDeviceBuffer() { if (p) (void)hipFree(p); }
    hipError_t init(size_t n) { return hipMalloc((void**)&p, n * sizeof(T)); }
    T* release() { T* q = p; p = nullptr; return q; }
};

// ---- the logs of a closed loop: DEVICE blocks of one row per tick that the loop's kernels write, copied to the host after the loop's one host
// wait.  The whole-loop logs of brov_closed_loop_ex / _dob, the one-chunk device logs of brov_closed_loop_track and the six logs of the fleet's
// loops are all declared, allocated, initialised, delivered and freed here -------------------------------------------------------------------
struct LoopLog {
    struct Column {
        size_t elem, width, lead;   // bytes per element (double or int32_t), elements per instance per tick, rows ahead of tick 0
        void* host;                 // where deliver() copies the column; null: a device-only column
        bool wanted;                // a host destination was given, or the column is device-only: alloc() gives it a block
        char* dev;
    };
    std::vector<Column> cols;
    size_t B = 0, n = 0;
    DeviceAllocs mem;
    LoopLog() { cols.reserve(6); }   // one host allocation for the columns of any loop
    LoopLog(const LoopLog&) = delete;
    ~LoopLog() { mem.free_all(); }   // on every way out
    // declares a column of T and returns its index; without a host destination it exists only as a device-only column.  The state column of
    // a whole loop has lead = 1: the start state ahead of the states after every tick
    template <typename T>
    int column(size_t width, T* host, size_t lead = 0, bool device_only = false) {
        static_assert(sizeof(T) == sizeof(double) || sizeof(T) == sizeof(int32_t), "a log column holds double or int32_t");
        cols.push_back(Column{sizeof(T), width, lead, host, host != nullptr || device_only, nullptr});
        return (int)cols.size() - 1;
    }
    size_t row_bytes(const Column& c) const { return B * c.width * c.elem; }
    // the wanted columns for `n_` ticks of `B_` instances (a column without a row gets no block)
    int alloc(size_t B_, size_t n_, std::string& err, const std::string& pre) {
        B = B_; n = n_;
        for (Column& c : cols) {
            if (!c.wanted || n + c.lead == 0) continue;
            if (int rc = mem.alloc(&c.dev, (n + c.lead) * row_bytes(c), err)) { err = pre + err; return rc; }
        }
        return BROV_OK;
    }
    // row `j` (tick j of the run) of column `c`, whose element type is T; null when the column was not asked for
    template <typename T>
    T* row(int c, size_t j) const { return cols[c].dev ? (T*)(cols[c].dev + (j + cols[c].lead) * row_bytes(cols[c])) : nullptr; }
    // enqueues the initialisation on `st`: zeros into column `zero_col` (-1: none; the caller names it only where nothing will write its rows)
    // and `start` into the lead rows
    int init(const void* start, int zero_col, hipStream_t st, std::string& err, const std::string& pre) {
        hipError_t e = hipSuccess;
        if (zero_col >= 0 && cols[zero_col].dev) e = hipMemsetAsync(cols[zero_col].dev, 0, (n + cols[zero_col].lead) * row_bytes(cols[zero_col]), st);
        for (const Column& c : cols)
            if (c.dev && c.lead && e == hipSuccess) e = hipMemcpyAsync(c.dev, start, c.lead * row_bytes(c), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) return BROV_OK;
        (void)hipGetLastError();
        err = pre + "log initialisation failed";
        return BROV_ERR_HIP;
    }
    // after the loop's host wait: the columns to their host destinations, from a loop that completed alone (rc, which is handed on) -- a
    // failing call leaves the caller's arrays as they were
    int deliver(int rc, std::string& err, const std::string& pre) {
        if (rc != BROV_OK) return rc;
        for (const Column& c : cols)
            if (c.dev && c.host && hipMemcpy(c.host, c.dev, (n + c.lead) * row_bytes(c), hipMemcpyDeviceToHost) != hipSuccess) rc = BROV_ERR_HIP;
        if (rc != BROV_OK) { (void)hipGetLastError(); err = pre + "copying the logs back failed"; }
        return rc;
    }
};
// the end of a closed loop: its one host wait, then a launch error nobody has picked up (its text behind `pre`), then the code
inline int finish_loop(hipStream_t st, int rc, std::string& err, const std::string& pre) {
    hipError_t e = hipStreamSynchronize(st);
    if (rc == BROV_OK && e == hipSuccess) e = hipGetLastError();
    if (rc == BROV_OK && e != hipSuccess) { err = pre + hipGetErrorString(e); rc = BROV_ERR_HIP; }
    return rc;
}

}  // namespace brov
