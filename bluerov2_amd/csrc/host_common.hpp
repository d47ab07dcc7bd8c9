// host_common.hpp -- the host-side scaffolding every device object of the C ABI is built from (brov_solver, brov_ekf, brov_rls, brov_track,
// brov_group): the HIP error check, the "is this device usable" test of the create calls, an owner of device allocations, a two-event kernel
// timer and a scoped temporary device buffer.  Host code only, header only.  Each component keeps its OWN thread-local error string and its own
// brov_*_last_error(): a failing observer call must not overwrite brov_last_error(), so everything here that reports takes the string to write.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
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

// ---- what a component that is laid over a solver (brov_fleet) asks of it beyond the public accessors, without the side effects of the
// public hand-outs (brov_params_device marks the plant's copy of the parameters stale); filled by nmpc_api.hip -------------------------------
struct SolverView {
    int device = 0;
    const double* par = nullptr;          // [B][N+1][16] model parameters in force
    bool cand_set = false;                // candidate shape parameters are resident (brov_set_candidate_params_host)
    hipStream_t last_stream = nullptr;    // where the solver enqueued last: the stream its closed loops run on
};
SolverView solver_view(const brov_solver* s);

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

}  // namespace brov
