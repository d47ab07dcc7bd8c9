// fleet_api.hip -- host side of the fleet planning loop (include/bluerov2_nmpc.h, brov_fleet_*; kernels: fleet_kernel.hip).  A brov_fleet is
// laid over a brov_solver of batch B = V * C and owns what the solver has no place for: the V vehicle states, the input each vehicle was
// given last, the winners of the last select, the vehicles' true parameters, the world-frame wrench every vehicle is under (brov_vehicle_wrench_*:
// the solver's generator at batch V, instance index v), the water the vehicles move in (brov_vehicle_current_*, brov_vehicle_coriolis_*: the
// solver's two stages at batch V; kernel: fleet_water_kernel.hip) and what a disturbance observer of batch V is fed from (brov_vehicle_observe).  It
// reaches the solver through its public calls (brov_order_stream, brov_set_yref_candidates, brov_solve, the DEVICE pointers) and solver_view()
// of host_common.hpp, the observer through brov_ekf_update_device and brov_ekf_mpc_p_device.  The inter-vehicle clearance term
// (brov_clearance_*; kernels: clearance_kernel.hip) lives here too: its plan, buffers and statistics are the fleet's, and a step with the term on
// re-scores the records ahead of the select and publishes the plan behind it.  So does the stand-off term (brov_standoff_*; kernels:
// standoff_kernel.hip), which prices the candidates by their closest approach to the solver's scene (solver_scene(), standoff_kernel.hpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "clearance_kernel.hpp"
#include "coriolis_source.hpp"
#include "current_source.hpp"
#include "fleet_kernel.hpp"
#include "host_common.hpp"
#include "nmpc_device.hpp"
#include "standoff_kernel.hpp"
#include "wrench_source.hpp"

using namespace brov;

static thread_local std::string g_fleet_err;
#define HIPCHK(call) BROV_HIPCHK(g_fleet_err, call)

struct brov_fleet {
    brov_solver* s = nullptr;
    int device = 0, V = 0, C = 0, B = 0, N = 0;
    double* xv = nullptr;              // [V][12] measured vehicle states
    double* u_hold = nullptr;          // [V][4] input applied last (zeros after reset)
    double* pplant = nullptr;          // [V][16] true parameters (brov_fleet_set_plant_params_host)
    bool pplant_set = false;
    int32_t* winner = nullptr;         // [V] of the last select
    int32_t* status = nullptr;         // [V] of the last step
    brov_result* winner_rec = nullptr; // [V] brov_fleet_select_host
    brov_result* stage_rec = nullptr;  // [B] brov_fleet_select_host: the caller's records on the device
    // world-frame wrench of the vehicles (brov_vehicle_wrench_*) at batch V, its buffers reserved at create.  Its counter: steps since the last
    // reset.  Its eval buffer also holds the wrench of the tick in flight where no log row takes it
    WrenchSource wr;
    // the water the vehicles move in (brov_vehicle_current_*, brov_vehicle_coriolis_*): the solver's two stages at batch V, ticked by wr.tick
    CurrentSource cu;
    CoriolisSource co;
    double* co_pp = nullptr;           // [V][16] brov_vehicle_coriolis_eval_host while pplant is unset: the parameters the plant would read
    double* vprev = nullptr;           // [V][6] velocities at the last brov_vehicle_observe (zeros after reset)
    double *y12 = nullptr, *thrust = nullptr, *acc = nullptr;   // [V][12], [V][6], [V][6] the observer's inputs
    // the inter-vehicle clearance term (brov_clearance_*), its buffers reserved at create; off by default
    struct Clearance {
        bool on = false;
        double radius = 0.0, weight = 0.0, r2 = 0.0;
        int shift = 0, slices = 1;
        double* plan = nullptr;        // [N+1][V][3] stage-major: the positions of the path every vehicle committed to last
        double* part = nullptr;        // [kClearanceMaxSlices][B], [slices][B] used: the distance kernel's minima per slice of the peer range
        double* d2min = nullptr;       // [B] of the last step or brov_clearance_eval_host
        brov_result* rec = nullptr;    // [B] the re-scored records a step selects from
        double *last_d2 = nullptr, *min_d2 = nullptr;   // [V] statistics
        int32_t* below = nullptr;      // [V]
        KernelTimer timer;             // around the last distance kernel
    } cl;
    // the stand-off term (brov_standoff_*): the candidates kept clear of the solver's scene; its buffers reserved at create; off by default
    struct Standoff {
        bool on = false;
        double radius = 0.0, weight = 0.0, r2 = 0.0, reach = 0.0, reach2 = 0.0;
        int first = 1;
        double* part = nullptr;        // [N+1][B], [N+1-first][B] used: the distance kernel's minima per stage
        double* s2 = nullptr;          // [B] of the last step or brov_standoff_eval_host
        brov_result* rec = nullptr;    // [B] the re-scored records a step selects from
        long long* visits = nullptr;   // [B][2] brov_standoff_eval_host
        double *last_s2 = nullptr, *min_s2 = nullptr;   // [V] statistics
        int32_t* below = nullptr;      // [V]
        KernelTimer timer;             // around the last distance kernel
    } so;
    hipStream_t last_stream = nullptr;
    KernelTimer timer;                 // around the last select kernel
    hipEvent_t ev_done = nullptr;      // behind the last enqueued work
    bool done_valid = false;
    DeviceAllocs mem;
};

extern "C" const char* brov_fleet_last_error(void) { return g_fleet_err.c_str(); }
// What the entry point `who` hands to the wrench source (CallCtx, host_common.hpp); its wait: the device, and the host wait for a step in flight
// that may still read the generator's buffers
static int wrench_wait(brov_fleet* f) {
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipStreamSynchronize(f->last_stream));
    return BROV_OK;
}
static CallCtx call_ctx(brov_fleet* f, const char* who) { return {[f] { return wrench_wait(f); }, f->mem, g_fleet_err, who}; }

extern "C" void brov_fleet_destroy(brov_fleet* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    (void)hipStreamSynchronize(f->last_stream);
    f->mem.free_all();
    f->wr.destroy();
    f->cu.destroy();
    f->co.destroy();
    f->timer.destroy();
    f->cl.timer.destroy();
    f->so.timer.destroy();
    if (f->ev_done) (void)hipEventDestroy(f->ev_done);
    delete f;
}

extern "C" int brov_fleet_vehicles(const brov_fleet* f) { return f ? f->V : 0; }
extern "C" int brov_fleet_candidates(const brov_fleet* f) { return f ? f->C : 0; }

// work on `st` behind whatever the fleet enqueued last, without a host wait
static int order_behind(brov_fleet* f, hipStream_t st) {
    if (f->done_valid && f->last_stream != st) HIPCHK(hipStreamWaitEvent(st, f->ev_done, 0));
    return BROV_OK;
}
static int enqueued_on(brov_fleet* f, hipStream_t st) {
    HIPCHK(hipEventRecord(f->ev_done, st));
    f->done_valid = true;
    f->last_stream = st;
    return BROV_OK;
}
// `st` behind the solver's last stream and behind the fleet's own
static int order_both(brov_fleet* f, hipStream_t st, const char* who) {
    if (brov_order_stream(f->s, st) != BROV_OK) {
        g_fleet_err = std::string(who) + ": could not order behind the solver's last stream";
        return BROV_ERR_HIP;
    }
    return order_behind(f, st);
}
// host-side wait for everything that may still touch the fleet's or the solver's arrays
static int wait_all(brov_fleet* f, const char* who) {
    if (int rc = order_both(f, nullptr, who)) return rc;
    HIPCHK(hipStreamSynchronize(f->last_stream));
    HIPCHK(hipStreamSynchronize(nullptr));
    return BROV_OK;
}

// the plan of a fleet that has not planned yet: every vehicle stays where it is (every stage := the position of xv[v], HOST [V][12]);
// the statistics as before the first step.  The caller has waited for everything that may touch the buffers.
static int clearance_hold(brov_fleet* f, const double* xv) {
    const size_t V = (size_t)f->V, K = (size_t)f->N + 1;
    std::vector<double> plan(K * V * 3);
    for (size_t k = 0; k < K; k++)
        for (size_t v = 0; v < V; v++)
            for (size_t j = 0; j < 3; j++) plan[(k * V + v) * 3 + j] = xv[v * 12 + j];
    HIPCHK(hipMemcpy(f->cl.plan, plan.data(), plan.size() * sizeof(double), hipMemcpyHostToDevice));
    const std::vector<double> last(V, -1.0), lowest(V, std::numeric_limits<double>::infinity());
    HIPCHK(hipMemcpy(f->cl.last_d2, last.data(), V * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(f->cl.min_d2, lowest.data(), V * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(f->cl.below, 0, V * sizeof(int32_t)));
    // the stand-off term's statistics are reset where the clearance term's are
    HIPCHK(hipMemcpy(f->so.last_s2, last.data(), V * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(f->so.min_s2, lowest.data(), V * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(f->so.below, 0, V * sizeof(int32_t)));
    return BROV_OK;
}

extern "C" int brov_fleet_reset(brov_fleet* f) {
    if (!f) { g_fleet_err = "brov_fleet_reset: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(f->device));
    if (int rc = wait_all(f, "brov_fleet_reset")) return rc;
    HIPCHK(hipMemset(f->u_hold, 0, (size_t)f->V * 4 * sizeof(double)));
    HIPCHK(hipMemset(f->status, 0, (size_t)f->V * sizeof(int32_t)));
    HIPCHK(hipMemset(f->winner, 0xff, (size_t)f->V * sizeof(int32_t)));   // -1: no select yet
    HIPCHK(hipMemset(f->vprev, 0, (size_t)f->V * 6 * sizeof(double)));
    // xv[v] := x0 of candidate 0 of group v
    HIPCHK(hipMemcpy2D(f->xv, 12 * sizeof(double), brov_x0_device(f->s), (size_t)f->C * 12 * sizeof(double), 12 * sizeof(double), (size_t)f->V,
                       hipMemcpyDeviceToDevice));
    f->wr.tick = 0;
    if (int rc = f->cu.rewind(g_fleet_err)) return rc;
    if (int rc = f->co.rewind(g_fleet_err)) return rc;
    std::vector<double> xv((size_t)f->V * 12);
    HIPCHK(hipMemcpy(xv.data(), f->xv, xv.size() * sizeof(double), hipMemcpyDeviceToHost));
    return clearance_hold(f, xv.data());
}

extern "C" int brov_fleet_create(brov_fleet** out, brov_solver* s, int candidates) {
    if (!out || !s) { g_fleet_err = "brov_fleet_create: null argument"; return BROV_ERR_ARG; }
    *out = nullptr;
    const int B = brov_batch(s);
    if (candidates < 1 || candidates > B || B % candidates != 0) {
        g_fleet_err = "brov_fleet_create: the solver's batch of " + std::to_string(B) + " is not a whole number of groups of " +
                      std::to_string(candidates) + " candidates (needs 1 <= candidates <= B and B % candidates == 0)";
        return BROV_ERR_ARG;
    }
    const SolverView sv = solver_view(s);
    HIPCHK(hipSetDevice(sv.device));
    brov_fleet* f = new brov_fleet();
    f->s = s; f->device = sv.device; f->B = B; f->C = candidates; f->V = B / candidates; f->N = brov_horizon(s);
    const size_t V = (size_t)f->V;
    int rc = f->mem.alloc(&f->xv, V * 12, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->u_hold, V * 4, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->pplant, V * 16, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->winner, V, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->status, V, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->winner_rec, V, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->stage_rec, (size_t)B, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->vprev, V * 6, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->y12, V * 12, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->thrust, V * 6, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->acc, V * 6, g_fleet_err);
    f->cl.slices = clearance_slices(B, f->V);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->cl.plan, ((size_t)f->N + 1) * V * 3, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->cl.part, (size_t)kClearanceMaxSlices * B, g_fleet_err);   // (brov_clearance_dev_set_slices may raise the count)
    if (rc == BROV_OK) rc = f->mem.alloc(&f->cl.d2min, (size_t)B, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->cl.rec, (size_t)B, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->cl.last_d2, V, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->cl.min_d2, V, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->cl.below, V, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->so.part, ((size_t)f->N + 1) * B, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->so.s2, (size_t)B, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->so.rec, (size_t)B, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->so.visits, (size_t)B * 2, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->so.last_s2, V, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->so.min_s2, V, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->so.below, V, g_fleet_err);
    if (rc == BROV_OK) rc = f->mem.alloc(&f->co_pp, V * 16, g_fleet_err);
    f->wr.B = f->cu.B = f->co.B = V;
    if (rc == BROV_OK) rc = f->wr.reserve(call_ctx(f, "brov_fleet_create"));   // eager: a step reads the eval buffer without a host wait
    if (rc != BROV_OK) { g_fleet_err = "brov_fleet_create: " + g_fleet_err; brov_fleet_destroy(f); return rc; }
    if (f->timer.create() != hipSuccess || f->cl.timer.create() != hipSuccess || f->so.timer.create() != hipSuccess || hipEventCreateWithFlags(&f->ev_done, hipEventDisableTiming) != hipSuccess) {
        g_fleet_err = "brov_fleet_create: device initialisation failed";
        brov_fleet_destroy(f);
        return BROV_ERR_HIP;
    }
    if ((rc = brov_fleet_reset(f)) != BROV_OK) { brov_fleet_destroy(f); return rc; }
    *out = f;
    return BROV_OK;
}

extern "C" int brov_fleet_set_state_host(brov_fleet* f, const double* xv) {
    if (!f || !xv) { g_fleet_err = "brov_fleet_set_state_host: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(f->device));
    if (int rc = wait_all(f, "brov_fleet_set_state_host")) return rc;
    HIPCHK(hipMemcpy(f->xv, xv, (size_t)f->V * 12 * sizeof(double), hipMemcpyHostToDevice));
    launch_fleet_bcast(f->xv, f->V, f->C, brov_x0_device(f->s), nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));
    return clearance_hold(f, xv);
}

extern "C" int brov_fleet_get_state_host(brov_fleet* f, double* xv) {
    if (!f || !xv) { g_fleet_err = "brov_fleet_get_state_host: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipStreamSynchronize(f->last_stream));
    HIPCHK(hipMemcpy(xv, f->xv, (size_t)f->V * 12 * sizeof(double), hipMemcpyDeviceToHost));
    return BROV_OK;
}

extern "C" int brov_fleet_set_plant_params_host(brov_fleet* f, const double* p) {
    if (!f) { g_fleet_err = "brov_fleet_set_plant_params_host: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipStreamSynchronize(f->last_stream));   // a plant step in flight may still read the buffer
    if (p) HIPCHK(hipMemcpy(f->pplant, p, (size_t)f->V * 16 * sizeof(double), hipMemcpyHostToDevice));
    f->pplant_set = p != nullptr;
    return BROV_OK;
}

// the select on `st`, timed; the caller has ordered the stream
static int select_on(brov_fleet* f, const brov_result* rec, int32_t* winner, brov_result* winner_rec, hipStream_t st) {
    HIPCHK(f->timer.start(st));
    launch_fleet_select(rec, f->V, f->C, winner, winner_rec, st);
    HIPCHK(hipGetLastError());
    HIPCHK(f->timer.stop(st));
    return BROV_OK;
}

extern "C" int brov_fleet_select_device(brov_fleet* f, const brov_result* rec, int32_t* winner, brov_result* winner_rec, void* stream) {
    if (!f || !winner) { g_fleet_err = "brov_fleet_select_device: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = order_both(f, st, "brov_fleet_select_device")) return rc;
    if (int rc = select_on(f, rec ? rec : brov_results_device(f->s), winner, winner_rec, st)) return rc;
    return enqueued_on(f, st);
}

extern "C" int brov_fleet_select_host(brov_fleet* f, const brov_result* rec_host, int32_t* winner, brov_result* winner_rec) {
    if (!f || !winner) { g_fleet_err = "brov_fleet_select_host: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(f->device));
    if (int rc = wait_all(f, "brov_fleet_select_host")) return rc;   // the staging buffer and the winners may still be in use
    if (rec_host) HIPCHK(hipMemcpy(f->stage_rec, rec_host, (size_t)f->B * sizeof(brov_result), hipMemcpyHostToDevice));
    if (int rc = select_on(f, rec_host ? f->stage_rec : brov_results_device(f->s), f->winner, winner_rec ? f->winner_rec : nullptr, nullptr)) return rc;
    if (int rc = enqueued_on(f, nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(winner, f->winner, (size_t)f->V * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (winner_rec) HIPCHK(hipMemcpy(winner_rec, f->winner_rec, (size_t)f->V * sizeof(brov_result), hipMemcpyDeviceToHost));
    return BROV_OK;
}

// ---- the world-frame wrench of the vehicles: the solver's generator (plant_wrench.hip) at batch V, thin forwards to the one host side,
// wrench_source.hpp -------------------------------------------------------------------------------------------------------------------------
static int no_fleet(const char* who) { g_fleet_err = std::string(who) + ": null argument"; return BROV_ERR_ARG; }
extern "C" int brov_vehicle_wrench_constant_host(brov_fleet* f, const double* w) {
    return f ? f->wr.constant_host(w, call_ctx(f, "brov_vehicle_wrench_constant_host")) : no_fleet("brov_vehicle_wrench_constant_host");
}
extern "C" int brov_vehicle_wrench_periodic(brov_fleet* f, uint64_t seed, double scale, double phase0, double dphi, double tz_div) {
    if (!f) return no_fleet("brov_vehicle_wrench_periodic");
    return f->wr.periodic(seed, scale, phase0, dphi, tz_div, call_ctx(f, "brov_vehicle_wrench_periodic"));
}
extern "C" int brov_vehicle_wrench_table_host(brov_fleet* f, const double* tab, int rows, const double* gain) {
    return f ? f->wr.table_host(tab, rows, gain, call_ctx(f, "brov_vehicle_wrench_table_host")) : no_fleet("brov_vehicle_wrench_table_host");
}
extern "C" int brov_vehicle_wrench_off(brov_fleet* f) { return f ? f->wr.set_off() : no_fleet("brov_vehicle_wrench_off"); }
extern "C" int brov_vehicle_wrench_mode(const brov_fleet* f) { return f ? f->wr.mode() : BROV_WRENCH_OFF; }
extern "C" int brov_vehicle_wrench_seek(brov_fleet* f, int64_t tick) {
    return f ? f->wr.seek(tick, call_ctx(f, "brov_vehicle_wrench_seek")) : no_fleet("brov_vehicle_wrench_seek");
}
extern "C" int64_t brov_vehicle_wrench_tick(const brov_fleet* f) { return f ? (int64_t)f->wr.tick : 0; }
extern "C" int brov_vehicle_wrench_eval_host(brov_fleet* f, int64_t tick, double* w) {
    return f ? f->wr.eval_host(tick, w, f->last_stream, call_ctx(f, "brov_vehicle_wrench_eval_host")) : no_fleet("brov_vehicle_wrench_eval_host");
}

// ---- the water the vehicles move in: the solver's current (plant_current.hip's generator) and Coriolis stage (plant_coriolis.hip's force) at
// batch V, thin forwards to their one host side, current_source.hpp and coriolis_source.hpp; the tick is the fleet's step counter ----------------
extern "C" int brov_vehicle_current_constant_host(brov_fleet* f, const double* v) {
    return f ? f->cu.constant_host(v, call_ctx(f, "brov_vehicle_current_constant_host")) : no_fleet("brov_vehicle_current_constant_host");
}
extern "C" int brov_vehicle_current_table_host(brov_fleet* f, const double* tab, int rows, const double* gain) {
    return f ? f->cu.table_host(tab, rows, gain, call_ctx(f, "brov_vehicle_current_table_host")) : no_fleet("brov_vehicle_current_table_host");
}
extern "C" int brov_vehicle_current_gauss_markov_host(brov_fleet* f, uint64_t seed, const double* mean, const double* mu, const double* amp,
                                                      const double* lo, const double* hi, double step) {
    if (!f) return no_fleet("brov_vehicle_current_gauss_markov_host");
    return f->cu.gauss_markov_host(seed, mean, mu, amp, lo, hi, step, call_ctx(f, "brov_vehicle_current_gauss_markov_host"));
}
extern "C" int brov_vehicle_current_off(brov_fleet* f) { return f ? f->cu.set_off() : no_fleet("brov_vehicle_current_off"); }
extern "C" int brov_vehicle_current_mode(const brov_fleet* f) { return f ? f->cu.mode() : BROV_CURRENT_OFF; }
extern "C" int brov_vehicle_current_eval_host(brov_fleet* f, int64_t tick, double* v) {
    return f ? f->cu.eval_host(tick, v, f->last_stream, call_ctx(f, "brov_vehicle_current_eval_host")) : no_fleet("brov_vehicle_current_eval_host");
}
extern "C" int brov_vehicle_current_get_state_host(brov_fleet* f, double* v) {
    if (!f) return no_fleet("brov_vehicle_current_get_state_host");
    return f->cu.get_state_host(f->wr.tick, v, f->last_stream, call_ctx(f, "brov_vehicle_current_get_state_host"));
}
extern "C" int brov_vehicle_current_set_state_host(brov_fleet* f, const double* v) {
    return f ? f->cu.set_state_host(v, call_ctx(f, "brov_vehicle_current_set_state_host")) : no_fleet("brov_vehicle_current_set_state_host");
}
extern "C" int brov_vehicle_current_last_host(brov_fleet* f, double* v) {
    return f ? f->cu.last_host(v, call_ctx(f, "brov_vehicle_current_last_host")) : no_fleet("brov_vehicle_current_last_host");
}
extern "C" int brov_vehicle_coriolis_set(brov_fleet* f, int terms, double ka, double ma) {
    return f ? f->co.set(terms, ka, ma, call_ctx(f, "brov_vehicle_coriolis_set")) : no_fleet("brov_vehicle_coriolis_set");
}
extern "C" int brov_vehicle_coriolis_off(brov_fleet* f) { return f ? f->co.set_off() : no_fleet("brov_vehicle_coriolis_off"); }
extern "C" int brov_vehicle_coriolis_terms(const brov_fleet* f) { return f ? f->co.terms() : 0; }
extern "C" int brov_vehicle_coriolis_get(const brov_fleet* f, int* terms, double* ka, double* ma) {
    if (!f) return no_fleet("brov_vehicle_coriolis_get");
    return f->co.get(terms, ka, ma, call_ctx(const_cast<brov_fleet*>(f), "brov_vehicle_coriolis_get"));
}
extern "C" int brov_vehicle_coriolis_eval_host(brov_fleet* f, const double* x, const double* vc, double* c) {
    if (!f) return no_fleet("brov_vehicle_coriolis_eval_host");
    if (!x || !c) return call_ctx(f, "brov_vehicle_coriolis_eval_host").refuse("null argument");
    HIPCHK(hipSetDevice(f->device));
    const double* pp = f->pplant;   // the parameters the next step of the fleet's plant would read
    if (!f->pplant_set) {           // stage 0 of candidate 0 of every group, as they stand once the solver's stream has drained
        if (int rc = wait_all(f, "brov_vehicle_coriolis_eval_host")) return rc;
        HIPCHK(hipMemcpy2D(f->co_pp, 16 * sizeof(double), solver_view(f->s).par, (size_t)f->C * (f->N + 1) * 16 * sizeof(double), 16 * sizeof(double),
                           (size_t)f->V, hipMemcpyDeviceToDevice));
        pp = f->co_pp;
    }
    return f->co.eval_host(x, vc, c, pp, f->last_stream, call_ctx(f, "brov_vehicle_coriolis_eval_host"));
}
extern "C" int brov_vehicle_coriolis_last_host(brov_fleet* f, double* c) {
    return f ? f->co.last_host(c, call_ctx(f, "brov_vehicle_coriolis_last_host")) : no_fleet("brov_vehicle_coriolis_last_host");
}

// what the plant of the fleet does not model: the vehicles' wrench is the fleet's (brov_vehicle_wrench_*), indexed
// by the vehicle; the solver's is indexed by the instance v * C + c, and so are the solver's current and Coriolis stage, which mean nothing
// here either: the vehicles' water is the fleet's (brov_vehicle_current_*, brov_vehicle_coriolis_*).  Nor does its broadcast of the vehicles' states know the solver's
// sensor stage (brov_sensor_*): the candidates would be solved at a measured state nothing refreshes
static int plant_modes_ok(const brov_fleet* f, const char* who) {
    if (brov_plant_wrench_mode(f->s) != BROV_WRENCH_OFF) {
        g_fleet_err = std::string(who) + ": a plant wrench mode of the solver is in force (brov_plant_wrench_*); the vehicles' wrench is set with "
                      "brov_vehicle_wrench_*";
        return BROV_ERR_ARG;
    }
    if (brov_thruster_enabled(f->s) == 1) {
        g_fleet_err = std::string(who) + ": the thruster stage of the solver's plant is on (brov_thruster_set_host); the fleet's plant gives every "
                      "vehicle the wrench it asked for";
        return BROV_ERR_ARG;
    }
    if (brov_delay_enabled(f->s) == 1) {
        g_fleet_err = std::string(who) + ": the delay stage of the solver's plant is on (brov_delay_set_host); the fleet's plant applies every "
                      "winner's command on the tick it was solved";
        return BROV_ERR_ARG;
    }
    if (brov_rotor_enabled(f->s) == 1) {
        g_fleet_err = std::string(who) + ": the rotor stage of the solver's plant is on (brov_rotor_set_host); the fleet's plant turns every "
                      "winner's command into force on the tick it was solved";
        return BROV_ERR_ARG;
    }
    if (brov_curve_enabled(f->s) == 1) {
        g_fleet_err = std::string(who) + ": the thrust-curve stage of the solver's plant is on (brov_curve_set_host); the fleet's plant turns "
                      "every winner's command into force linearly";
        return BROV_ERR_ARG;
    }
    if (brov_current_mode(f->s) != BROV_CURRENT_OFF) {
        g_fleet_err = std::string(who) + ": an ocean current of the solver's plant is in force (brov_current_*); the fleet's plant integrates "
                      "the vehicles in still water";
        return BROV_ERR_ARG;
    }
    if (brov_coriolis_terms(f->s) != 0) {
        g_fleet_err = std::string(who) + ": the Coriolis stage of the solver's plant is on (brov_coriolis_set); the fleet's plant integrates "
                      "the OCP model, which has no such forces";
        return BROV_ERR_ARG;
    }
    if (brov_sensor_enabled(f->s) == 1) {
        g_fleet_err = std::string(who) + ": the sensor stage of the solver is on (brov_sensor_set_host); the fleet hands every candidate its "
                      "vehicle's true state";
        return BROV_ERR_ARG;
    }
    if (brov_imu_enabled(f->s) == 1) {
        g_fleet_err = std::string(who) + ": the IMU stage of the solver's plant is on (brov_imu_set_host); the fleet's plant steps the vehicles, "
                      "which that stage never samples";
        return BROV_ERR_ARG;
    }
    if (brov_inspect_enabled(f->s) == 1) {
        g_fleet_err = std::string(who) + ": the inspection controller of the solver is on (brov_inspect_set_host); it writes the records the fleet "
                      "selects among";
        return BROV_ERR_ARG;
    }
    if (brov_dist6_enabled(f->s) == 1) {
        g_fleet_err = std::string(who) + ": the 6-disturbance variant is on (brov_enable_dist6); the fleet's plant integrates the shipped model";
        return BROV_ERR_ARG;
    }
    return BROV_OK;
}

// the two clearance kernels on `st` (ordered by the caller) against the plan as it stands: the distance kernel, timed, then the fold of its
// slices into d2min and, with `out`, the re-scored records
static int clearance_on(brov_fleet* f, const double* x, const brov_result* rec, double* d2min, brov_result* out, hipStream_t st) {
    HIPCHK(f->cl.timer.start(st));
    launch_clearance_dist(x, f->cl.plan, f->B, f->V, f->C, f->N, f->cl.shift, f->cl.slices, f->cl.part, st);
    HIPCHK(hipGetLastError());
    HIPCHK(f->cl.timer.stop(st));
    launch_clearance_rescore(f->cl.part, f->cl.slices, f->B, rec, f->cl.r2, f->cl.weight, d2min, out, st);
    HIPCHK(hipGetLastError());
    return BROV_OK;
}

// may a step run as far as the stand-off term goes?  With the term on the solver's scene must still hold a box or a mesh
static int standoff_ok(const brov_fleet* f, const char* who) {
    if (!f->so.on || !solver_scene(f->s).empty()) return BROV_OK;
    g_fleet_err = std::string(who) + ": the stand-off term is on and the solver's scene holds neither a box nor a mesh (brov_range_set_scene_host, "
                  "brov_mesh_set_host); brov_standoff_off turns the term off";
    return BROV_ERR_ARG;
}

// the stand-off kernels on `st` (ordered by the caller) against the solver's scene as it stands: the distance kernel, timed, then the fold of
// its slices into s2 and, with `out`, the re-scored records (the clearance term's kernel: the layout and the rule are the same).  Without
// `visits` every stage is a slice of the grid; with them one lane walks all stages of its candidate and counts
static int standoff_on(brov_fleet* f, const double* x, const brov_result* rec, double* s2, brov_result* out, long long* visits, hipStream_t st) {
    const SceneView sc = solver_scene(f->s);
    const int per = visits ? f->N + 1 : 1;
    HIPCHK(f->so.timer.start(st));
    launch_standoff_dist(x, sc.boxes, sc.mesh, f->B, f->N, f->so.first, per, f->so.reach2, f->so.part, visits, st);
    HIPCHK(hipGetLastError());
    HIPCHK(f->so.timer.stop(st));
    launch_clearance_rescore(f->so.part, standoff_slices(f->N, f->so.first, per), f->B, rec, f->so.r2, f->so.weight, s2, out, st);
    HIPCHK(hipGetLastError());
    return BROV_OK;
}

// select + plant + broadcast on `st` (ordered by the caller, who has checked the wrench and the current tick), with optional DEVICE log rows of
// this tick.  Under a wrench mode the wrench of the tick is evaluated into wlog's row (or the source's eval buffer): the plant's input and the
// log row are one.  In moving water (a current mode in force or the Coriolis stage on) the plant is fleet_plant_water_kernel, which evaluates
// the current itself; else every launch is the one of a fleet without the two stages.
static int step_on(brov_fleet* f, const brov_result* rec, double dt, int substeps, double* xlog, double* ulog, int32_t* stlog, int32_t* winlog,
                   double* wlog, hipStream_t st) {
    if (!rec) rec = brov_results_device(f->s);
    if (f->cl.on) {   // the candidates priced by their clearance from the other vehicles' plans: the select, the plant and the logs see these records
        if (int rc = clearance_on(f, brov_x_device(f->s), rec, f->cl.d2min, f->cl.rec, st)) return rc;
        rec = f->cl.rec;
    }
    if (f->so.on) {   // ... and by their closest approach to the scene: the stand-off term re-scores what the clearance term hands on
        if (int rc = standoff_on(f, brov_x_device(f->s), rec, f->so.s2, f->so.rec, nullptr, st)) return rc;
        rec = f->so.rec;
    }
    if (int rc = select_on(f, rec, f->winner, nullptr, st)) return rc;
    FleetPlantArgs a;
    a.V = f->V; a.C = f->C; a.xv = f->xv; a.res = rec; a.winner = f->winner;
    if (f->pplant_set) { a.pp = f->pplant; a.pp_stride = 16; }
    else { a.pp = solver_view(f->s).par; a.pp_stride = (long long)f->C * (f->N + 1) * 16; }   // stage 0 of candidate 0, as it stands now
    a.dt = dt; a.substeps = substeps; a.u_hold = f->u_hold; a.status = f->status;
    a.xlog = xlog; a.ulog = ulog; a.stlog = stlog; a.winlog = winlog;
    const bool water = !f->cu.off() || f->co.on;
    double* wv = f->wr.off() ? nullptr : (wlog ? wlog : f->wr.eval);
    if (wv) {
        launch_wrench_eval(f->wr.gen, f->V, f->wr.tick, wv, st);
        HIPCHK(hipGetLastError());
    }
    if (water) launch_fleet_plant_water(a, wv, f->cu.gen, f->co.gen, f->wr.tick, st);
    else if (wv) launch_fleet_plant_wrench(a, wv, st);
    else launch_fleet_plant(a, st);
    HIPCHK(hipGetLastError());
    launch_fleet_bcast(f->xv, f->V, f->C, brov_x0_device(f->s), st);
    HIPCHK(hipGetLastError());
    if (f->cl.on) {   // behind the select: the winners' paths are the plans the next tick keeps clear of
        launch_clearance_publish(brov_x_device(f->s), f->winner, f->cl.d2min, f->V, f->C, f->N, f->cl.shift, f->cl.r2, f->cl.plan, f->cl.last_d2,
                                 f->cl.min_d2, f->cl.below, st);
        HIPCHK(hipGetLastError());
    }
    if (f->so.on) {
        launch_standoff_stats(f->winner, f->so.s2, f->V, f->C, f->so.r2, f->so.last_s2, f->so.min_s2, f->so.below, st);
        HIPCHK(hipGetLastError());
    }
    f->wr.tick++;
    return enqueued_on(f, st);
}

extern "C" int brov_fleet_step(brov_fleet* f, const brov_result* rec, double dt, int substeps, void* stream) {
    if (!f || !(dt > 0.0) || !std::isfinite(dt) || substeps < 1) {
        g_fleet_err = "brov_fleet_step: bad argument (needs dt > 0 and substeps >= 1)";
        return BROV_ERR_ARG;
    }
    if (int rc = plant_modes_ok(f, "brov_fleet_step")) return rc;
    if (int rc = standoff_ok(f, "brov_fleet_step")) return rc;
    if (int rc = f->wr.steps_ok(1, call_ctx(f, "brov_fleet_step"))) return rc;
    if (int rc = f->cu.steps_ok(f->wr.tick, 1, call_ctx(f, "brov_fleet_step"))) return rc;
    HIPCHK(hipSetDevice(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = order_both(f, st, "brov_fleet_step")) return rc;
    return step_on(f, rec, dt, substeps, nullptr, nullptr, nullptr, nullptr, nullptr, st);
}

extern "C" int brov_fleet_get_last_host(brov_fleet* f, double* u, int32_t* status, int32_t* winner) {
    if (!f) { g_fleet_err = "brov_fleet_get_last_host: null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipStreamSynchronize(f->last_stream));
    if (u) HIPCHK(hipMemcpy(u, f->u_hold, (size_t)f->V * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, f->status, (size_t)f->V * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (winner) HIPCHK(hipMemcpy(winner, f->winner, (size_t)f->V * sizeof(int32_t), hipMemcpyDeviceToHost));
    return BROV_OK;
}

// ---- the disturbance observer in the fleet's loop -----------------------------------------------------------------------------------------
static int observer_ok(const brov_fleet* f, const brov_ekf* e, const char* who) {
    if (brov_ekf_batch(e) != f->V) {
        g_fleet_err = std::string(who) + ": the observer's batch of " + std::to_string(brov_ekf_batch(e)) + " is not the fleet's " +
                      std::to_string(f->V) + " vehicles";
        return BROV_ERR_ARG;
    }
    return BROV_OK;
}
// the estimate goes to the CONTROLLER; a fleet whose plant reads the controller's stage-0 parameters would be fed it back
static int apply_ok(const brov_fleet* f, const char* who) {
    if (!f->pplant_set) {
        g_fleet_err = std::string(who) + ": the fleet's plant parameters are unset (brov_fleet_set_plant_params_host): its plant reads the "
                      "controller's stage-0 parameters, the estimate would be fed back into the plant";
        return BROV_ERR_ARG;
    }
    if (brov_dist6_enabled(f->s) == 1) {
        g_fleet_err = std::string(who) + ": the 6-disturbance variant is on (brov_enable_dist6); the fleet hands off the four disturbances of the shipped model";
        return BROV_ERR_ARG;
    }
    return BROV_OK;
}
// on `st`, ordered by the caller
static int observe_on(brov_fleet* f, brov_ekf* e, double dt, const char* who, hipStream_t st) {
    launch_fleet_observe_inputs(f->V, dt, f->xv, f->u_hold, f->vprev, f->thrust, f->y12, f->acc, st);
    HIPCHK(hipGetLastError());
    if (int rc = brov_ekf_update_device(e, f->thrust, f->y12, f->acc, st)) {
        g_fleet_err = std::string(who) + ": " + brov_ekf_last_error();
        return rc;
    }
    return enqueued_on(f, st);
}
static int apply_on(brov_fleet* f, brov_ekf* e, hipStream_t st) {
    launch_fleet_apply(f->V, f->C, f->N + 1, brov_ekf_mpc_p_device(e), brov_params_device(f->s), st);
    HIPCHK(hipGetLastError());
    return enqueued_on(f, st);
}

extern "C" int brov_vehicle_observe(brov_fleet* f, brov_ekf* e, double dt, void* stream) {
    if (!f || !e || !(dt > 0.0) || !std::isfinite(dt)) {
        g_fleet_err = "brov_vehicle_observe: bad argument (needs a fleet, an observer and dt > 0)";
        return BROV_ERR_ARG;
    }
    if (int rc = observer_ok(f, e, "brov_vehicle_observe")) return rc;
    HIPCHK(hipSetDevice(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = order_both(f, st, "brov_vehicle_observe")) return rc;
    return observe_on(f, e, dt, "brov_vehicle_observe", st);
}

extern "C" int brov_vehicle_apply_estimate(brov_fleet* f, brov_ekf* e, void* stream) {
    if (!f || !e) { g_fleet_err = "brov_vehicle_apply_estimate: null argument"; return BROV_ERR_ARG; }
    if (int rc = observer_ok(f, e, "brov_vehicle_apply_estimate")) return rc;
    if (int rc = apply_ok(f, "brov_vehicle_apply_estimate")) return rc;
    HIPCHK(hipSetDevice(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = order_both(f, st, "brov_vehicle_apply_estimate")) return rc;
    return apply_on(f, e, st);
}

// the planning loop of brov_closed_loop_fleet (e == nullptr, no w_log, no est_log) and brov_closed_loop_fleet_dob
static int fleet_loop(brov_fleet* f, brov_ekf* e, const char* who, int ticks, double t0, double dt_ref, double dt_node, double dt, int substeps,
                      double* u_log, double* x_log, int32_t* st_log, int32_t* win_log, double* w_log, double* est_log) {
    const std::string pre = std::string(who) + ": ";
    if (!f || ticks < 0 || !std::isfinite(t0) || !std::isfinite(dt_ref) || !std::isfinite(dt_node) || !(dt > 0.0) || !std::isfinite(dt) ||
        substeps < 1) {
        g_fleet_err = pre + "bad argument (needs ticks >= 0, finite t0, dt_ref and dt_node, dt > 0, substeps >= 1)";
        return BROV_ERR_ARG;
    }
    if (!e && est_log) { g_fleet_err = pre + "an estimate log without an observer"; return BROV_ERR_ARG; }
    if (int rc = plant_modes_ok(f, who)) return rc;
    if (int rc = standoff_ok(f, who)) return rc;
    if (e) {
        if (int rc = observer_ok(f, e, who)) return rc;
        if (int rc = apply_ok(f, who)) return rc;
    }
    if (int rc = f->wr.steps_ok(ticks, call_ctx(f, who))) return rc;
    if (int rc = f->cu.steps_ok(f->wr.tick, ticks, call_ctx(f, who))) return rc;
    const SolverView sv = solver_view(f->s);
    if (!sv.cand_set) {
        g_fleet_err = pre + "no candidate parameters (brov_set_candidate_params_host)";
        return BROV_ERR_ARG;
    }
    HIPCHK(hipSetDevice(f->device));
    hipStream_t st = sv.last_stream;
    // DEVICE logs for the whole run (LoopLog, host_common.hpp), a column per HOST log asked for; the states behind the start state
    LoopLog L;
    const int X = L.column(12, x_log, 1), U = L.column(4, u_log), ST = L.column(1, st_log), WIN = L.column(1, win_log), W = L.column(6, w_log),
              EST = L.column(6, est_log);
    int rc = L.alloc((size_t)f->V, (size_t)ticks, g_fleet_err, pre);
    if (rc == BROV_OK) rc = order_both(f, st, who);
    if (rc == BROV_OK) rc = L.init(f->xv, f->wr.off() ? W : -1, st, g_fleet_err, pre);   // (mode OFF: no wrench, nothing writes its log)
    for (int k = 0; k < ticks && rc == BROV_OK; k++) {
        rc = brov_set_yref_candidates(f->s, t0 + k * dt_ref, dt_node, st);
        if (rc == BROV_OK) rc = brov_solve(f->s, st);
        if (rc != BROV_OK) { g_fleet_err = pre + brov_last_error(); break; }
        rc = step_on(f, nullptr, dt, substeps, L.row<double>(X, k), L.row<double>(U, k), L.row<int32_t>(ST, k), L.row<int32_t>(WIN, k),
                     L.row<double>(W, k), st);
        if (e && rc == BROV_OK) rc = observe_on(f, e, dt, who, st);
        if (e && rc == BROV_OK) rc = apply_on(f, e, st);
        double* est = L.row<double>(EST, k);
        if (rc == BROV_OK && est) {
            launch_gather_cols(brov_ekf_x_device(e), f->V, 18, 12, 6, est, st);
            if (hipGetLastError() != hipSuccess) { g_fleet_err = pre + "gathering the estimate failed"; rc = BROV_ERR_HIP; }
        }
    }
    return L.deliver(finish_loop(st, rc, g_fleet_err, pre), g_fleet_err, pre);
}

extern "C" int brov_closed_loop_fleet(brov_fleet* f, int ticks, double t0, double dt_ref, double dt_node, double dt, int substeps, double* u_log,
                                      double* x_log, int32_t* st_log, int32_t* win_log) {
    return fleet_loop(f, nullptr, "brov_closed_loop_fleet", ticks, t0, dt_ref, dt_node, dt, substeps, u_log, x_log, st_log, win_log, nullptr, nullptr);
}

extern "C" int brov_closed_loop_fleet_dob(brov_fleet* f, brov_ekf* e, int ticks, double t0, double dt_ref, double dt_node, double dt, int substeps,
                                          double* u_log, double* x_log, int32_t* st_log, int32_t* win_log, double* w_log, double* est_log) {
    return fleet_loop(f, e, "brov_closed_loop_fleet_dob", ticks, t0, dt_ref, dt_node, dt, substeps, u_log, x_log, st_log, win_log, w_log, est_log);
}

extern "C" int brov_fleet_last_seconds(brov_fleet* f, double* select_seconds) {
    if (!f || !select_seconds || !f->timer.valid) { g_fleet_err = "brov_fleet_last_seconds: no select yet"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(f->device));
    return f->timer.seconds(select_seconds, g_fleet_err);
}

// ---- the inter-vehicle clearance term (kernels: clearance_kernel.hip) ---------------------------------------------
static int no_clearance(const char* who) { g_fleet_err = std::string(who) + ": null argument"; return BROV_ERR_ARG; }

extern "C" int brov_clearance_set(brov_fleet* f, double radius, double weight, int shift) {
    if (!f) return no_clearance("brov_clearance_set");
    const double r2 = radius * radius;   // what the kernels compare against: a radius whose square overflows or underflows is refused
    if (!(radius > 0.0) || !std::isfinite(radius) || !(r2 > 0.0) || !std::isfinite(r2) || !(weight > 0.0) || shift < 0 || shift > f->N) {
        g_fleet_err = "brov_clearance_set: bad argument (needs a finite radius > 0 whose square is finite and > 0, a weight > 0 that may be +Inf, "
                      "and 0 <= shift <= N = " + std::to_string(f->N) + ")";
        return BROV_ERR_ARG;
    }
    f->cl.radius = radius; f->cl.weight = weight; f->cl.shift = shift;
    f->cl.r2 = r2;
    f->cl.on = true;
    return BROV_OK;
}

extern "C" int brov_clearance_off(brov_fleet* f) {
    if (!f) return no_clearance("brov_clearance_off");
    f->cl.on = false;
    return BROV_OK;
}

extern "C" int brov_clearance_enabled(const brov_fleet* f) { return f && f->cl.on ? 1 : 0; }

extern "C" int brov_clearance_dev_set_slices(brov_fleet* f, int slices) {
    if (!f) return no_clearance("brov_clearance_dev_set_slices");
    if (slices < 0 || slices > kClearanceMaxSlices) {
        g_fleet_err = "brov_clearance_dev_set_slices: bad argument (needs 0 <= slices <= " + std::to_string(kClearanceMaxSlices) + ", 0: the default)";
        return BROV_ERR_ARG;
    }
    f->cl.slices = slices ? slices : clearance_slices(f->B, f->V);   // a launch takes the count by value: no wait
    return BROV_OK;
}
extern "C" int brov_clearance_dev_slices(const brov_fleet* f) { return f ? f->cl.slices : 0; }

// HOST [V][N+1][3] <-> the device's stage-major [N+1][V][3]
extern "C" int brov_clearance_set_plan_host(brov_fleet* f, const double* plan) {
    if (!f || !plan) return no_clearance("brov_clearance_set_plan_host");
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipStreamSynchronize(f->last_stream));   // a step in flight may still read or write the plan
    const size_t V = (size_t)f->V, K = (size_t)f->N + 1;
    std::vector<double> t(K * V * 3);
    for (size_t v = 0; v < V; v++)
        for (size_t k = 0; k < K; k++)
            for (size_t j = 0; j < 3; j++) t[(k * V + v) * 3 + j] = plan[(v * K + k) * 3 + j];
    HIPCHK(hipMemcpy(f->cl.plan, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    return BROV_OK;
}

extern "C" int brov_clearance_get_plan_host(brov_fleet* f, double* plan) {
    if (!f || !plan) return no_clearance("brov_clearance_get_plan_host");
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipStreamSynchronize(f->last_stream));
    const size_t V = (size_t)f->V, K = (size_t)f->N + 1;
    std::vector<double> t(K * V * 3);
    HIPCHK(hipMemcpy(t.data(), f->cl.plan, t.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t v = 0; v < V; v++)
        for (size_t k = 0; k < K; k++)
            for (size_t j = 0; j < 3; j++) plan[(v * K + k) * 3 + j] = t[(k * V + v) * 3 + j];
    return BROV_OK;
}

static int clearance_is_set(const brov_fleet* f, const char* who) {
    if (f->cl.on) return BROV_OK;
    g_fleet_err = std::string(who) + ": the clearance term is off (brov_clearance_set gives the radius, the weight and the shift)";
    return BROV_ERR_ARG;
}

extern "C" int brov_clearance_eval_device(brov_fleet* f, const double* x, const brov_result* rec, double* d2min, brov_result* out, void* stream) {
    if (!f || !d2min) return no_clearance("brov_clearance_eval_device");
    if (int rc = clearance_is_set(f, "brov_clearance_eval_device")) return rc;
    HIPCHK(hipSetDevice(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = order_both(f, st, "brov_clearance_eval_device")) return rc;
    if (int rc = clearance_on(f, x ? x : brov_x_device(f->s), rec ? rec : brov_results_device(f->s), d2min, out, st)) return rc;
    return enqueued_on(f, st);
}

extern "C" int brov_clearance_eval_host(brov_fleet* f, const brov_result* rec_host, double* d2min, brov_result* out) {
    if (!f || !d2min) return no_clearance("brov_clearance_eval_host");
    if (int rc = clearance_is_set(f, "brov_clearance_eval_host")) return rc;
    HIPCHK(hipSetDevice(f->device));
    if (int rc = wait_all(f, "brov_clearance_eval_host")) return rc;   // the staging buffer and the fleet's own d2min may still be in use
    if (rec_host) HIPCHK(hipMemcpy(f->stage_rec, rec_host, (size_t)f->B * sizeof(brov_result), hipMemcpyHostToDevice));
    if (int rc = clearance_on(f, brov_x_device(f->s), rec_host ? f->stage_rec : brov_results_device(f->s), f->cl.d2min, out ? f->cl.rec : nullptr,
                              nullptr))
        return rc;
    if (int rc = enqueued_on(f, nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(d2min, f->cl.d2min, (size_t)f->B * sizeof(double), hipMemcpyDeviceToHost));
    if (out) HIPCHK(hipMemcpy(out, f->cl.rec, (size_t)f->B * sizeof(brov_result), hipMemcpyDeviceToHost));
    return BROV_OK;
}

extern "C" int brov_clearance_get_stats_host(brov_fleet* f, double* last_d2, double* min_d2, int32_t* below) {
    if (!f) return no_clearance("brov_clearance_get_stats_host");
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipStreamSynchronize(f->last_stream));
    const size_t V = (size_t)f->V;
    if (last_d2) HIPCHK(hipMemcpy(last_d2, f->cl.last_d2, V * sizeof(double), hipMemcpyDeviceToHost));
    if (min_d2) HIPCHK(hipMemcpy(min_d2, f->cl.min_d2, V * sizeof(double), hipMemcpyDeviceToHost));
    if (below) HIPCHK(hipMemcpy(below, f->cl.below, V * sizeof(int32_t), hipMemcpyDeviceToHost));
    return BROV_OK;
}

extern "C" int brov_clearance_last_seconds(brov_fleet* f, double* seconds) {
    if (!f || !seconds || !f->cl.timer.valid) { g_fleet_err = "brov_clearance_last_seconds: no distance kernel yet"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(f->device));
    return f->cl.timer.seconds(seconds, g_fleet_err);
}

// ---- the stand-off term (kernels: standoff_kernel.hip) -------------------------------------------------------------
static int no_standoff(const char* who) { g_fleet_err = std::string(who) + ": null argument"; return BROV_ERR_ARG; }

extern "C" int brov_standoff_set(brov_fleet* f, double radius, double weight, double reach, int first) {
    if (!f) return no_standoff("brov_standoff_set");
    const double r2 = radius * radius;   // what the kernels compare against: a radius whose square overflows or underflows is refused
    if (!(radius > 0.0) || !std::isfinite(radius) || !(r2 > 0.0) || !std::isfinite(r2) || !(weight > 0.0) || !(reach >= radius) || first < 0 ||
        first > f->N) {
        g_fleet_err = "brov_standoff_set: bad argument (needs a finite radius > 0 whose square is finite and > 0, a weight > 0 that may be +Inf, "
                      "a reach >= radius that may be +Inf, and 0 <= first <= N = " + std::to_string(f->N) + ")";
        return BROV_ERR_ARG;
    }
    if (solver_scene(f->s).empty()) {
        g_fleet_err = "brov_standoff_set: the solver's scene holds neither a box nor a mesh (brov_range_set_scene_host, brov_mesh_set_host)";
        return BROV_ERR_ARG;
    }
    f->so.radius = radius; f->so.weight = weight; f->so.reach = reach; f->so.first = first;
    f->so.r2 = r2;
    f->so.reach2 = reach * reach;   // formed once, here; +Inf for a reach that is
    f->so.on = true;
    return BROV_OK;
}

extern "C" int brov_standoff_off(brov_fleet* f) {
    if (!f) return no_standoff("brov_standoff_off");
    f->so.on = false;
    return BROV_OK;
}

extern "C" int brov_standoff_enabled(const brov_fleet* f) { return f && f->so.on ? 1 : 0; }

// the term is on and the scene still holds something to keep clear of
static int standoff_is_set(const brov_fleet* f, const char* who) {
    if (f->so.on) return standoff_ok(f, who);
    g_fleet_err = std::string(who) + ": the stand-off term is off (brov_standoff_set gives the radius, the weight, the reach and the first stage)";
    return BROV_ERR_ARG;
}

extern "C" int brov_standoff_eval_device(brov_fleet* f, const double* x, const brov_result* rec, double* s2, brov_result* out, int64_t* visits,
                                         void* stream) {
    if (!f || !s2) return no_standoff("brov_standoff_eval_device");
    if (int rc = standoff_is_set(f, "brov_standoff_eval_device")) return rc;
    HIPCHK(hipSetDevice(f->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = order_both(f, st, "brov_standoff_eval_device")) return rc;
    if (int rc = standoff_on(f, x ? x : brov_x_device(f->s), rec ? rec : brov_results_device(f->s), s2, out, (long long*)visits, st)) return rc;
    return enqueued_on(f, st);
}

extern "C" int brov_standoff_eval_host(brov_fleet* f, const brov_result* rec_host, double* s2, brov_result* out, int64_t* visits) {
    if (!f || !s2) return no_standoff("brov_standoff_eval_host");
    if (int rc = standoff_is_set(f, "brov_standoff_eval_host")) return rc;
    HIPCHK(hipSetDevice(f->device));
    if (int rc = wait_all(f, "brov_standoff_eval_host")) return rc;   // the staging buffer and the fleet's own s2 may still be in use
    if (rec_host) HIPCHK(hipMemcpy(f->stage_rec, rec_host, (size_t)f->B * sizeof(brov_result), hipMemcpyHostToDevice));
    if (int rc = standoff_on(f, brov_x_device(f->s), rec_host ? f->stage_rec : brov_results_device(f->s), f->so.s2, out ? f->so.rec : nullptr,
                             visits ? f->so.visits : nullptr, nullptr))
        return rc;
    if (int rc = enqueued_on(f, nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(s2, f->so.s2, (size_t)f->B * sizeof(double), hipMemcpyDeviceToHost));
    if (out) HIPCHK(hipMemcpy(out, f->so.rec, (size_t)f->B * sizeof(brov_result), hipMemcpyDeviceToHost));
    if (visits) HIPCHK(hipMemcpy(visits, f->so.visits, (size_t)f->B * 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return BROV_OK;
}

extern "C" int brov_standoff_get_stats_host(brov_fleet* f, double* last_s2, double* min_s2, int32_t* below) {
    if (!f) return no_standoff("brov_standoff_get_stats_host");
    HIPCHK(hipSetDevice(f->device));
    HIPCHK(hipStreamSynchronize(f->last_stream));
    const size_t V = (size_t)f->V;
    if (last_s2) HIPCHK(hipMemcpy(last_s2, f->so.last_s2, V * sizeof(double), hipMemcpyDeviceToHost));
    if (min_s2) HIPCHK(hipMemcpy(min_s2, f->so.min_s2, V * sizeof(double), hipMemcpyDeviceToHost));
    if (below) HIPCHK(hipMemcpy(below, f->so.below, V * sizeof(int32_t), hipMemcpyDeviceToHost));
    return BROV_OK;
}

extern "C" int brov_standoff_last_seconds(brov_fleet* f, double* seconds) {
    if (!f || !seconds || !f->so.timer.valid) { g_fleet_err = "brov_standoff_last_seconds: no distance kernel yet"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(f->device));
    return f->so.timer.seconds(seconds, g_fleet_err);
}
