// nmpc_api.hip -- host side of the batched solver: owns the HBM state of B OCP instances and implements the C ABI of
// include/bluerov2_nmpc.h (each entry point there cites the reference call it replaces).  No CPU compute path: without a
// usable HIP device every entry point fails with BROV_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <atomic>
#include <chrono>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"
#include "select_device.hpp"
#include "solver_plant.hpp"
#include "standoff_kernel.hpp"

using namespace brov;

#define kTickMailboxMaxBatch 64          /* brov_tick_host: up to this many instances deliver their records through the host mailbox */

static thread_local std::string g_err;
extern "C" const char* brov_last_error(void) { return g_err.c_str(); }

#define HIPCHK(call) BROV_HIPCHK(g_err, call)

// What ONE launch reads and writes in place of the solver's own arrays (null: those): a local of brov_tick_host, handed down to solve_phase /
// make_params.  A zero-copy tick's kernel reads the inputs passed with it straight from the pinned staging buffer (no copy command ahead of
// it); the records go to the host mailbox of that tick (device-visible pinned memory).
struct LaunchInputs {
    const double *x0 = nullptr, *yref = nullptr, *par = nullptr;
    brov_result* mail = nullptr;
    int32_t* mail_flag = nullptr;    // sequence words the host polls (null with `mail` set: a large batch, the host waits for the launch)
    int32_t mail_seq = 0;
    bool reads_pinned = false;       // the kernel reads the pinned inputs: no need to order it behind the refresh copies of an earlier tick
};
// The pinned staging buffer of brov_tick_host, offsets in doubles: input set 0 (x0 | shared window | stage parameters) | records | sequence
// words | input set 1.  Ticks that copy their arguments in alternate between the two input sets; set 0 is the one brov_tick_buffers hands out.
struct TickLayout {
    size_t n_x0, n_y, n_p, n_r, n_f;
    TickLayout(size_t B, size_t N)
        : n_x0(B * 12), n_y((N + 1) * 16), n_p(B * (N + 1) * 16), n_r((B * sizeof(brov_result) + 7) / 8), n_f((B * sizeof(int32_t) + 7) / 8) {}
    size_t inputs() const { return n_x0 + n_y + n_p; }
    size_t x0(int set) const { return set ? inputs() + n_r + n_f : 0; }
    size_t window(int set) const { return x0(set) + n_x0; }
    size_t params(int set) const { return window(set) + n_y; }
    size_t records() const { return inputs(); }
    size_t seq_words() const { return inputs() + n_r; }
    size_t total() const { return 2 * inputs() + n_r + n_f; }
};
// Everything that belongs to brov_tick_host's transport alone, all of it created on first use
struct TickChannel {
    hipStream_t stream = nullptr;        // the solver's own non-blocking stream
    double* pin = nullptr;               // pinned staging buffer (TickLayout)
    size_t pin_doubles = 0;
    hipEvent_t ev_up = nullptr;          // a preparation tick (rti_phase 1): its uploads have left the pinned staging buffer
    hipEvent_t ev_tick = nullptr;        // ticks with inputs read in place: the kernel's end (neither the host nor the next tick's kernel waits for the copies behind it)
    hipEvent_t ev_pre = nullptr;         // large batches: recorded AHEAD of the tick's kernel -- its refresh copies run next to the kernel, not behind it
    hipStream_t copy_stream = nullptr;   // ... those copies (pinned staging buffer -> the device arrays every other entry point works on) run here, behind ev_tick
    hipEvent_t ev_copy = nullptr;        // ... and end here (alias of the ev_set[] recorded last)
    hipEvent_t ev_set[2] = {nullptr, nullptr};   // the refresh copies out of input set 0 / 1 of the pinned staging buffer (see stage_inputs)
    bool set_pending[2] = {false, false};
    int pin_sel = 0;                     // input set the last copying tick used
    bool buffers_out = false;            // brov_tick_buffers has handed set 0 out
    bool copies_pending = false;         // ev_copy recorded and not yet waited for by the host
    int copy_mask = 0;                   // ... which device arrays those copies write: 1 x0, 2 shared window, 4 stage parameters
    int32_t mail_seq = 0;                // sequence number of the last mailbox tick
    double tick_us[5] = {0, 0, 0, 0, 0};   // BROV_TICK_BREAKDOWN=1: host time of the last brov_tick_host by part (brov_dev_tick_breakdown)
    // nothing of a tick may still be in flight when the solver's memory goes: the tail of its kernel, the input copies behind it
    void drain() { for (hipStream_t q : {stream, copy_stream}) if (q) hipStreamSynchronize(q); }
    void destroy() {
        if (pin) hipHostFree(pin);
        if (copy_stream) hipStreamDestroy(copy_stream);
        for (hipEvent_t e : {ev_tick, ev_pre, ev_up, ev_set[0], ev_set[1]}) if (e) hipEventDestroy(e);
        if (stream) hipStreamDestroy(stream);
    }
};

struct brov_solver {
    int device = 0, B = 0, N = 0;
    brov_opts opts{};
    bool yref_shared = false;
    const double* yref_view = nullptr;   // shared window = rows of the resident trajectory table, used in place (no copy)
    int traj_line = -1, traj_ncols = 0;  // the shared window in force was built from this row of the table by brov_set_yref_from_traj (-1: by something else)
    // device buffers
    double *x0 = nullptr, *yref = nullptr, *yref_sh = nullptr, *par = nullptr;
    double *x = nullptr, *u = nullptr, *pi = nullptr, *lam = nullptr;
    double *BA = nullptr, *bvec = nullptr, *kktp = nullptr;
    double *Ks = nullptr, *Kt = nullptr, *Mt = nullptr, *Pb = nullptr, *kff = nullptr, *vhat = nullptr, *ipm = nullptr,
           *dxb = nullptr, *cst = nullptr;
    brov_result* res = nullptr;
    int* best = nullptr;
    double* traj = nullptr;
    int traj_rows = 0;
    double* scratch3 = nullptr;  // [3][B] candidate parameters
    double* par_rp = nullptr;    // 6-disturbance variant: roll / pitch disturbance moments [B][N+1][2] (allocated by brov_enable_dist6)
    bool dist6 = false;
    SolverPlant plant;           // the simulated plant (solver_plant.hpp): its parameters, wrench, thruster and sensor stages, its step counter
    bool cand_set = false;       // candidate shape parameters resident in scratch3
    int cand_kind = 0;
    bool dump_lin = false;
    int* lines = nullptr;        // [B]
    DeviceAllocs mem;            // every buffer above that is not named in brov_destroy
    hipStream_t last_stream = nullptr;
    bool timing = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool ev_valid = false;
    int last_family = 0;             // kernel family of the last solve (FAM_*)
    int cus = 256;                   // compute units of the device, queried once in brov_create
    double* ws = nullptr;        // windowed kernel: per-block parking images
    int32_t* counter = nullptr;
    unsigned win_count = 0;           // windowed launches so far: which of the two hand-out counters the next one uses
    int win_blocks = 0, win_L = 0;
    double* ws_split = nullptr;      // fused-kernel horizons, at most one instance per CU: per-instance workspace of the resident kernel's split launches (rti_phase 1 / 2)
    int alt_blocks = 0, alt_L = 0;   // parallel-in-time rounds (pit_rounds_stages): the resident configuration a solve may use instead
    int prep_path = 0;               // the last rti_phase-1 call: 1 streaming pair (linearisation in HBM), 2 resident split (factorised LDS image parked), 3 the latter, invalidated by a setter
    unsigned long long* dbg = nullptr;
    // general grid (streaming kernels): per-stage time steps and / or a separate stage-0 weight
    std::vector<double> ts_host;     // N time steps, empty = uniform
    double W0_host[16] = {0};
    bool has_W0 = false;
    double* tsv = nullptr;           // device [N]
    double* wst = nullptr;           // device [N+1][16] scaled weights per stage
    int32_t* sched = nullptr;        // work ordering: 3 rotating buffers of 64 class counters | lists | pos[B] (qp_kernel.hip, sched_map)
    unsigned sched_tick = 0;
    TickChannel tick;                // brov_tick_host's transport; sync_last / order_behind_last wait for the refresh copies it leaves running
    bool pit_ran = false;            // the last solve launched rti_pit_kernel
    int32_t* pit_done = nullptr;     // [B]: written by rti_pit_kernel (parallel-in-time step-0 solve), read by the resident kernel launched behind it
    DevKnobs k;                     // development knobs (BROV_* environment), read once in brov_create: no getenv on the path of a solve
};

// The solver's development knobs: A/B switches and test hooks, all of them BROV_* environment variables.  Read ONCE per solver (brov_create;
// brov_dev_reload_knobs re-reads them for tests that flip a switch between two solves of one solver) -- a linear scan of the environment
// per variable has no place inside a 29 us feedback call (round 4 did up to 16 of them per solve).
static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
static DevKnobs read_knobs() {
    DevKnobs k;
    k.robust_pivot = env_int("BROV_ROBUST_PIVOT", 1);            // 0 off, 1 on demand (default), 2 every instance, 3 on demand without the KKT <= 1e6 limit
    if (const char* v = getenv("BROV_ROBUST_KKT_MAX")) k.robust_kkt_max = atof(v);   // entering KKT up to which the robust form is taken on demand
    k.partial_refactor = env_int("BROV_PARTIAL_REFACTOR", 1) != 0;
    k.mail_early = env_int("BROV_DEV_NO_EARLY_RECORD", 0) == 0;
    k.split_resident = env_int("BROV_SPLIT_RESIDENT", 1) != 0;
    k.pit = env_int("BROV_PIT", 1);                               // 0 off, 1 product rule, 2 every instance is tried
    k.split_parallel = env_int("BROV_SPLIT_PARALLEL", 1) != 0;
    k.pit_try = env_int("BROV_PIT_TRY", 1) != 0;
    k.pit_light = env_int("BROV_PIT_LIGHT", 1) != 0;
    k.tick_mailbox = env_int("BROV_TICK_MAILBOX", 1) != 0;
    k.tick_bulk = env_int("BROV_TICK_BULK", 1) != 0;
    k.tick_zerocopy = env_int("BROV_TICK_ZEROCOPY", 1) != 0;
    k.sched = env_int("BROV_SCHED", 1) != 0;
    k.force_windowed = env_int("BROV_DEV_FORCE_WINDOWED", 0) != 0;
    k.fused_waves = env_int("BROV_DEV_FUSED_WAVES", 0);           // 1 / 2: force a variant of the fused kernel (default by LDS size)
    k.lds_pad = env_int("BROV_DEV_LDS_PAD", 0);
    k.closed_loop_fused = env_int("BROV_CLOSED_LOOP_FUSED", 1) != 0;   // 0: brov_closed_loop as three launches per tick (A/B, tests)
    k.tick_breakdown = env_int("BROV_TICK_BREAKDOWN", 0) != 0;
    k.no_resident = env_int("BROV_DEV_NO_RESIDENT", 0) != 0;     // windows of <= 20 stages at every batch size (A/B, tests)
    k.win_blocks = env_int("BROV_DEV_WIN_BLOCKS", 0);             // >= 1: at most this many persistent blocks of the windowed kernel (tests)
    k.pit_rounds = env_int("BROV_PIT_ROUNDS", 1) != 0;            // 0: batches of one to two instances per CU stay on the windowed kernel
    k.win_long = env_int("BROV_DEV_WIN_LONG", 0) != 0;            // the long-horizon windowed instantiations at every horizon (A/B)
    return k;
}
extern "C" int brov_dev_reload_knobs(brov_solver* s) {
    if (!s) return BROV_ERR_ARG;
    const DevKnobs at_create = s->k;
    s->k = read_knobs();
    // the workspaces were allocated for the create-time values of the knobs that size them (plan_workspaces): those stay in force
    s->k.force_windowed = at_create.force_windowed; s->k.no_resident = at_create.no_resident;
    s->k.win_blocks = at_create.win_blocks; s->k.pit_rounds = at_create.pit_rounds;
    return BROV_OK;
}

extern "C" void brov_default_opts(brov_opts* o, int N, double Ts) {
    // /root/reference/bluerov2_dobmpc/scripts/c_generated_code/acados_solver_bluerov2.c:422-481 (W), :559-566 (bounds), :668
    static const double W[16] = {300, 480, 200, 10, 10, 200, 40, 40, 10, 10, 10, 10, 1, 1, 0.1, 0.05};
    std::memset(o, 0, sizeof(*o));
    o->N = N;
    o->Ts = Ts;
    for (int j = 0; j < 16; j++) o->W[j] = W[j];
    for (int j = 0; j < 12; j++) o->We[j] = W[j];
    for (int j = 0; j < 4; j++) { o->lbu[j] = -50.0; o->ubu[j] = 50.0; }
    o->qp_iter_max = 50;
    o->qp_tol_mu = 1e-7;
    o->qp_tol_stat = 1e-9;
    o->qp_early_exit = 1;
    o->kernel_path = BROV_PATH_AUTO;
    o->on_failure = BROV_ON_FAILURE_RESTART;
}

// what is wrong with a set of options (nullptr = nothing).  The QP must be strictly convex in the inputs (R > 0), the box must
// have an interior (the interior-point start divides by its width), limits and tolerances must be usable.
static const char* opts_problem(const brov_opts* o) {
    if (o->N < 1 || o->N > BROV_MAX_N) return "N out of range";
    if (!(o->Ts > 0.0) || !(o->Ts < 1e6)) return "Ts must be positive and finite";
    if (o->kernel_path < 0 || o->kernel_path > 2) return "kernel_path must be BROV_PATH_AUTO / _STREAMING / _FUSED";
    if (o->on_failure < 0 || o->on_failure > 1) return "on_failure must be BROV_ON_FAILURE_KEEP / _RESTART";
    for (int j = 0; j < 16; j++)
        if (!(o->W[j] >= 0.0) || !(o->W[j] < 1e300)) return "stage weights must be finite and >= 0";
    for (int j = 12; j < 16; j++)
        if (!(o->W[j] > 0.0)) return "input weights W[12..15] must be > 0 (strictly convex QP)";
    for (int j = 0; j < 12; j++)
        if (!(o->We[j] >= 0.0) || !(o->We[j] < 1e300)) return "terminal weights must be finite and >= 0";
    for (int j = 0; j < 4; j++)
        if (!(o->lbu[j] < o->ubu[j]) || !(o->lbu[j] > -1e300) || !(o->ubu[j] < 1e300)) return "input bounds need lbu < ubu, both finite";
    if (o->qp_iter_max < 1) return "qp_iter_max must be >= 1";
    if (!(o->qp_tol_mu > 0.0) || !(o->qp_tol_stat > 0.0)) return "qp tolerances must be > 0";
    return nullptr;
}

// a parked preparation (rti_phase 1 on the resident kernel's split launch) does not survive a call that changes what it factorised
static void invalidate_preparation(brov_solver* s) { if (s && s->prep_path == 2) s->prep_path = 3; }
// the shared window in force no longer names rows of the resident trajectory table
static void forget_traj_window(brov_solver* s) { s->yref_view = nullptr; s->traj_line = -1; }
// which LDS-resident kernels serve the solver's one-call step: the fused ones (whole horizon in an LDS slice, N <= 23) or the windowed ones
static bool serves_fused(const brov_solver* s) { return fused_supported(s->N) && !s->k.force_windowed; }
// ... and whether the windowed kernel runs in its large-batch configuration alone, the one that has a steps-per-launch variant
static bool serves_windowed_ticks(const brov_solver* s) { return s->ws != nullptr && !windowed_is_resident(s->win_L) && s->alt_L == 0; }

static bool general_grid(const brov_solver* s) { return !s->ts_host.empty() || s->has_W0; }
// per-stage time steps and scaled weights of the general grid: wst[i] = ts_i * (i == 0 ? W_0 : W) for i < N, wst[N] = [We | 0]
static int upload_grid(brov_solver* s) {
    if (!general_grid(s)) return BROV_OK;
    const int N = s->N;
    if (!s->tsv) {
        if (int rc = s->mem.alloc(&s->tsv, (size_t)N, g_err)) return rc;
        if (int rc = s->mem.alloc(&s->wst, (size_t)(N + 1) * 16, g_err)) return rc;
    }
    std::vector<double> ts(N), w((size_t)(N + 1) * 16, 0.0);
    for (int i = 0; i < N; i++) {
        ts[i] = s->ts_host.empty() ? s->opts.Ts : s->ts_host[i];
        const double* Wi = (i == 0 && s->has_W0) ? s->W0_host : s->opts.W;
        for (int j = 0; j < 16; j++) w[(size_t)i * 16 + j] = ts[i] * Wi[j];
    }
    for (int j = 0; j < 12; j++) w[(size_t)N * 16 + j] = s->opts.We[j];
    HIPCHK(hipMemcpy(s->tsv, ts.data(), ts.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->wst, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    return BROV_OK;
}
static int upload_cst(brov_solver* s) {
    double c[40];
    std::memset(c, 0, sizeof c);
    for (int j = 0; j < 16; j++) c[j] = s->opts.W[j];
    for (int j = 0; j < 12; j++) c[16 + j] = s->opts.We[j];
    for (int j = 0; j < 4; j++) { c[32 + j] = s->opts.lbu[j]; c[36 + j] = s->opts.ubu[j]; }
    HIPCHK(hipMemcpy(s->cst, c, sizeof c, hipMemcpyHostToDevice));
    return upload_grid(s);
}

extern "C" int brov_init_iterate_default(brov_solver* s) {
    invalidate_preparation(s);
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    const int B = s->B, N = s->N;
    std::vector<double> hx((size_t)B * (N + 1) * 12, 0.0);
    for (size_t k = 0; k < (size_t)B * (N + 1); k++) hx[k * 12 + 2] = -20.0;  // acados_solver_bluerov2.c:689-706
    HIPCHK(hipMemcpy(s->x, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(s->u, 0, (size_t)B * N * 4 * sizeof(double)));
    HIPCHK(hipMemset(s->pi, 0, (size_t)B * N * 12 * sizeof(double)));
    HIPCHK(hipMemset(s->lam, 0, (size_t)B * N * 8 * sizeof(double)));
    return BROV_OK;
}

// The workspaces of the LDS-resident kernels, decided at create from horizon, batch, CU count, path and the knobs that size them.
//   N <= 23 (fused kernels; BROV_DEV_FORCE_WINDOWED=1: none): no workspace for the one-call step.  rti_phase 1 / 2 run on the resident kernel's
//     split launches where its four waves all get a stage and the batch is at most one instance per CU: a workspace per instance (split).
//   N >= 24: the windowed kernel at every batch size.  Its RESIDENT mode -- one window = the whole horizon, one block per CU -- where that window's
//     LDS slice fits a CU's 160 KB, which is N <= 81, and the batch is at most one instance per CU; windows of <= 20 stages otherwise.  (Rounds 3-4
//     sent up to eight instances at N > 81 to the streaming pair, then as fast; since round 5 the windowed kernel is ahead there too -- one instance
//     at N = 82 / 128 / 160 / 256: 0.196 / 0.278 / 0.342 / 0.535 ms per step against 0.207 / 0.301 / 0.366 / 0.558, eight instances 0.198 / 0.281 /
//     0.344 / 0.539 against 0.241 / 0.343 / 0.421 / 0.686: scripts/dev/long_horizon_small_batches.py.)
//     The parallel-in-time kernel needs 244 doubles of the slice for itself and so serves the resident configuration up to N = 80.  Between one and
//     two instances per CU at 48 <= N <= 80 (alt: pit_rounds_stages) a solve it can serve runs it with one block and one workspace per instance, the
//     resident kernel behind it, instead of the windowed kernel: the workspace serves either.
//   BROV_PATH_STREAMING: none of them.
struct WorkspacePlan {
    int win_L = 0, win_blocks = 0;   // windowed kernel: stages per window, persistent blocks
    int alt_L = 0, alt_blocks = 0;   // ... the resident configuration a solve may take instead (0: none)
    size_t ws_doubles = 0;           // ... the workspace that serves both
    size_t split_doubles = 0;        // fused-kernel horizons: workspace of the resident split launches
};
static WorkspacePlan plan_workspaces(int N, int B, int cus, int kernel_path, const DevKnobs& k) {
    WorkspacePlan w;
    if (kernel_path == BROV_PATH_STREAMING) return w;
    if (fused_supported(N) && !k.force_windowed) {
        if (split_resident_horizon(N) && k.split_resident && B <= cus) w.split_doubles = (size_t)B * windowed_ws_doubles(N, N);
        return w;
    }
    w.win_L = windowed_stage_count(N, B, cus, k);
    w.win_blocks = windowed_blocks(B, w.win_L, cus, k);
    w.ws_doubles = (size_t)w.win_blocks * windowed_ws_doubles(N, w.win_L);
    if (!windowed_is_resident(w.win_L) && (w.alt_L = pit_rounds_stages(N, B, cus, k)) != 0) {   // one workspace per instance for rti_pit_kernel's blocks
        w.alt_blocks = windowed_blocks(B, w.alt_L, cus, k);
        const size_t alt = (size_t)B * windowed_ws_doubles(N, w.alt_L);
        w.ws_doubles = alt > w.ws_doubles ? alt : w.ws_doubles;
    }
    return w;
}

extern "C" int brov_create(brov_solver** out, int device, int B, const brov_opts* opts) {
    if (!out || !opts || B < 1) {
        g_err = "brov_create: bad argument";
        return BROV_ERR_ARG;
    }
    if (const char* why = opts_problem(opts)) {
        g_err = std::string("brov_create: ") + why;
        return BROV_ERR_ARG;
    }
    if (!usable_device(device)) {
        g_err = "brov_create: no usable HIP device (this library has no CPU fallback)";
        return BROV_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(device));
    {   // the kernels' dynamic-LDS limits on this device (once per device, checked): a refusal fails the create, not the first launch
        std::string why;
        if (int prc = prepare_kernels_on_device(&why)) { g_err = "brov_create: " + why; return prc; }
    }
    brov_solver* s = new brov_solver();
    s->device = device;
    s->B = B;
    s->N = opts->N;
    s->opts = *opts;
    const size_t N = opts->N, Bz = B;
    int rc = BROV_OK;
#define AL(ptr, n) if (rc == BROV_OK) rc = s->mem.alloc(&s->ptr, (n), g_err)
    // x0 | shared reference window | stage parameters in ONE allocation, in the order of brov_tick_host's staging buffer: a tick that
    // rewrites all three (the ROS node does) uploads them with one copy
    AL(x0, Bz * 12 + (size_t)(N + 1) * 16 + Bz * (N + 1) * 16);
    if (rc == BROV_OK) { s->yref_sh = s->x0 + Bz * 12; s->par = s->yref_sh + (size_t)(N + 1) * 16; }
    AL(yref, Bz * (N + 1) * 16);
    AL(x, Bz * (N + 1) * 12);
    AL(u, Bz * N * 4);
    AL(pi, Bz * N * 12);
    AL(lam, Bz * N * 8);
    AL(BA, Bz * N * 192);
    AL(bvec, Bz * N * 12);
    AL(kktp, Bz * N);
    AL(Ks, Bz * N * 64);
    AL(Kt, Bz * N * 192);
    AL(Mt, Bz * N * 64);
    AL(Pb, Bz * N * 12);
    AL(kff, Bz * N * 4);
    AL(vhat, Bz * N * 4);
    AL(ipm, Bz * IPM_NARR * N * 4);
    AL(dxb, Bz * (N + 1) * 12);
    AL(cst, 40);
    AL(res, Bz);
    AL(best, 2);
    AL(scratch3, 3 * Bz);
    AL(lines, Bz);
    AL(plant.pplant, Bz * 16);
    AL(counter, 64);   // two hand-out counters of the windowed kernel, 128 bytes apart, used alternately
    AL(pit_done, Bz);   // rti_pit_kernel's per-instance verdict
    AL(sched, 3 * (size_t)sched_buffer_ints_host(B));
    s->k = read_knobs();
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) s->cus = cus;
    const WorkspacePlan w = plan_workspaces(opts->N, B, s->cus, opts->kernel_path, s->k);
    s->win_L = w.win_L; s->win_blocks = w.win_blocks; s->alt_L = w.alt_L; s->alt_blocks = w.alt_blocks;
    if (w.ws_doubles) { AL(ws, w.ws_doubles); }
    if (w.split_doubles) { AL(ws_split, w.split_doubles); }
#undef AL
    if (rc != BROV_OK) { brov_destroy(s); return rc; }
    s->plant.init(B, opts->N, s->x0, s->res, s->par, &s->par_rp, &s->dist6);
    // create defaults: yref = 0, p = 0, x0 = [0,0,-20,0..] (acados_solver_bluerov2.c:355-364, 405-420, 520-527)
    hipMemset(s->yref, 0, Bz * (N + 1) * 16 * sizeof(double));
    hipMemset(s->yref_sh, 0, (N + 1) * 16 * sizeof(double));
    hipMemset(s->par, 0, Bz * (N + 1) * 16 * sizeof(double));
    hipMemset(s->res, 0, Bz * sizeof(brov_result));
    hipMemset(s->sched, 0, 3 * (size_t)sched_buffer_ints_host(B) * sizeof(int32_t));
    hipMemset(s->counter, 0, 64 * sizeof(int32_t));
    {
        std::vector<double> h0(Bz * 12, 0.0);
        for (size_t k = 0; k < Bz; k++) h0[k * 12 + 2] = -20.0;
        hipMemcpy(s->x0, h0.data(), h0.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    rc = upload_cst(s);
    if (rc == BROV_OK) rc = brov_init_iterate_default(s);
    if (rc != BROV_OK) { brov_destroy(s); return rc; }
    for (int k = 0; k < 3; k++) hipEventCreate(&s->ev[k]);
    *out = s;
    return BROV_OK;
}

extern "C" void brov_destroy(brov_solver* s) {
    if (!s) return;
    hipSetDevice(s->device);
    s->tick.drain();
    // (a caller's own stream is the caller's to drain -- it may not exist any more; hipFree below waits for the device in any case)
    s->mem.free_all();
    if (s->traj) hipFree(s->traj);
    s->plant.destroy();
    if (s->dbg) hipFree(s->dbg);
    s->tick.destroy();
    for (int k = 0; k < 3; k++)
        if (s->ev[k]) hipEventDestroy(s->ev[k]);
    delete s;
}

namespace brov {
SolverView solver_view(const brov_solver* s) {
    SolverView v;
    v.device = s->device; v.par = s->par; v.cand_set = s->cand_set; v.last_stream = s->last_stream;
    return v;
}
// the scene of the range stage as the next launch would be handed it (standoff_kernel.hpp): the fleet's stand-off term reads it per step
SceneView solver_scene(const brov_solver* s) {
    SceneView v;
    v.boxes = s->plant.in.scene; v.mesh = s->plant.in.mesh.dev;
    return v;
}
}  // namespace brov
extern "C" int brov_batch(const brov_solver* s) { return s ? s->B : 0; }
extern "C" int brov_horizon(const brov_solver* s) { return s ? s->N : 0; }
extern "C" size_t brov_device_bytes(const brov_solver* s) { return s ? s->mem.bytes : 0; }

// Stream ordering.  Everything a solver enqueues runs on the stream its caller names, and brov_tick_host uses the solver's own
// non-blocking stream and (mailbox path) returns while the tail of its kernel is still running.  A call that arrives on ANOTHER
// stream than the one last used would overlap that work and race on the iterate / work-ordering buffers / hand-out counters: the
// host waits for the earlier stream first.  Same stream (every loop in bench.py, the closed loop, tick after tick): a pointer
// comparison, no cost.
// host-side wait for everything the solver has in flight: the last stream, and the input copies a tick left running on the copy stream
static hipError_t sync_last(brov_solver* s) {
    hipError_t e = hipStreamSynchronize(s->last_stream);
    if (e == hipSuccess && s->tick.copies_pending) { e = hipEventSynchronize(s->tick.ev_copy); s->tick.copies_pending = false; }
    return e;
}
static int order_behind_last(brov_solver* s, hipStream_t st, bool reads_pinned = false) {
    if (s->last_stream != st) HIPCHK(hipStreamSynchronize(s->last_stream));
    // a tick's input copies (copy stream) write the device arrays this stream's next command may read or overwrite (reads_pinned: the launch
    // of a tick that reads its inputs in the pinned staging buffer instead, LaunchInputs)
    if (s->tick.copies_pending && !reads_pinned) HIPCHK(hipStreamWaitEvent(st, s->tick.ev_copy, 0));
    return BROV_OK;
}
extern "C" int brov_order_stream(brov_solver* s, void* stream) {
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    return order_behind_last(s, (hipStream_t)stream);
}

static int copy_in(brov_solver* s, double* dst, const double* src, size_t n, bool host, void* stream) {
    if (!s || !src) { g_err = "null argument"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(s->device));
    if (host) {
        // a solve may still be running on the caller's (possibly non-blocking) stream: the blocking copy on the null stream does not
        // wait for such a stream by itself
        HIPCHK(sync_last(s));
        HIPCHK(hipMemcpy(dst, src, n * sizeof(double), hipMemcpyHostToDevice));
    } else {
        if (int rc = order_behind_last(s, (hipStream_t)stream)) return rc;
        HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return BROV_OK;
}

// What the entry point `who` hands to the plant and its stages (CallCtx, host_common.hpp).  The solver has two waits: wrench_wait, for a plant step
// in flight that may still read the buffers; sensor_wait, for the whole device: a refresh may be enqueued on any stream a plant step was given
static int wrench_wait(brov_solver* s) {
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    return BROV_OK;
}
static int sensor_wait(brov_solver* s) {
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    s->tick.copies_pending = false;
    return BROV_OK;
}
static CallCtx call_ctx(brov_solver* s, const char* who, int (*wait)(brov_solver*) = wrench_wait) {
    return {[s, wait] { return wait(s); }, s->mem, g_err, who};
}

// the plant's true state; with the sensor stage on the measured state follows it: a forced refresh at the current index behind the copy
static int set_x0(brov_solver* s, const double* x0, bool host, void* st, const char* who) {
    if (s && x0) { if (int rc = s->plant.rewrite_ok(call_ctx(s, who))) return rc; }
    if (int rc = copy_in(s, s ? s->x0 : nullptr, x0, s ? (size_t)s->B * 12 : 0, host, st)) return rc;
    if (s->plant.rewritten(host ? s->last_stream : (hipStream_t)st)) HIPCHK(hipGetLastError());
    return BROV_OK;
}
extern "C" int brov_set_x0_host(brov_solver* s, const double* x0) { return set_x0(s, x0, true, nullptr, "brov_set_x0_host"); }
extern "C" int brov_set_x0_device(brov_solver* s, const double* x0, void* st) { return set_x0(s, x0, false, st, "brov_set_x0_device"); }

static const double* shared_window(const brov_solver* s) { return s->yref_view ? s->yref_view : s->yref_sh; }

static int set_yref(brov_solver* s, const double* y, int shared, bool host, void* st) {
    if (!s) return BROV_ERR_ARG;
    forget_traj_window(s);
    s->yref_shared = shared != 0;
    const size_t n = (size_t)(s->N + 1) * 16;
    return shared ? copy_in(s, s->yref_sh, y, n, host, st) : copy_in(s, s->yref, y, n * s->B, host, st);
}
extern "C" int brov_set_yref_host(brov_solver* s, const double* y, int shared) { return set_yref(s, y, shared, true, nullptr); }
extern "C" int brov_set_yref_device(brov_solver* s, const double* y, int shared, void* st) { return set_yref(s, y, shared, false, st); }

// one row of `w` doubles per instance, copied to every stage of the instance: dst [B][N1][w] <- src [B][w]
__global__ void bcast_rows_kernel(const double* __restrict__ src, double* __restrict__ dst, int B, int N1, int w) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)B * N1 * w) return;
    dst[t] = src[(t / ((size_t)N1 * w)) * w + t % w];
}
// per-stage rows [B][N+1][w] of the solver from the caller's [B][N+1][w] (per_stage) or [B][w] (one row for every stage of an instance)
static int set_stage_rows(brov_solver* s, double* dst, const double* p, int w, int per_stage, bool host, void* st) {
    const size_t N1 = s->N + 1, tot = (size_t)s->B * N1 * w;
    if (per_stage) return copy_in(s, dst, p, tot, host, st);
    HIPCHK(hipSetDevice(s->device));
    const double* src = p;
    ScopedDeviceBuffer<double> tmp;   // host rows: staged on the device until the kernel has read them
    if (!host) { if (int rc = order_behind_last(s, (hipStream_t)st)) return rc; }
    if (host) {
        HIPCHK(sync_last(s));
        HIPCHK(tmp.init((size_t)s->B * w));
        HIPCHK(hipMemcpy(tmp.p, p, (size_t)s->B * w * sizeof(double), hipMemcpyHostToDevice));
        src = tmp.p;
    }
    hipLaunchKernelGGL(bcast_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)st, src, dst, s->B, (int)N1, w);
    if (host) hipStreamSynchronize((hipStream_t)st);
    HIPCHK(hipGetLastError());
    return BROV_OK;
}
static int set_par(brov_solver* s, const double* p, int per_stage, bool host, void* st) {
    if (!s || !p) return BROV_ERR_ARG;
    s->plant.params_changed();
    return set_stage_rows(s, s->par, p, 16, per_stage, host, st);
}
extern "C" int brov_set_params_host(brov_solver* s, const double* p, int per_stage) { return set_par(s, p, per_stage, true, nullptr); }
extern "C" int brov_set_params_device(brov_solver* s, const double* p, int per_stage, void* st) { return set_par(s, p, per_stage, false, st); }

extern "C" int brov_set_param_stage_host(brov_solver* s, int inst, int stage, const double* p16) {
    if (!s || !p16 || inst < 0 || inst >= s->B || stage < 0 || stage > s->N) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    HIPCHK(hipMemcpy(s->par + ((size_t)inst * (s->N + 1) + stage) * 16, p16, 16 * sizeof(double), hipMemcpyHostToDevice));
    if (stage == 0) s->plant.params_changed();
    return BROV_OK;
}
// ---- boundary corners of the reference API: non-uniform grids and a separate stage-0 weight ------------------------------------
extern "C" int brov_set_time_steps(brov_solver* s, const double* ts) {
    invalidate_preparation(s);
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    if (!ts) s->ts_host.clear();
    else {
        for (int i = 0; i < s->N; i++)
            if (!(ts[i] > 0.0) || !(ts[i] < 1e6)) { g_err = "brov_set_time_steps: every time step must be positive and finite"; return BROV_ERR_ARG; }
        bool uniform = true;
        for (int i = 0; i < s->N; i++) uniform = uniform && std::fabs(ts[i] - ts[0]) <= 1e-12 * std::fabs(ts[0]);
        if (uniform) { s->ts_host.clear(); s->opts.Ts = ts[0]; }     // a uniform vector is the uniform grid: every kernel path stays open
        else s->ts_host.assign(ts, ts + s->N);
    }
    return upload_cst(s);
}
extern "C" int brov_set_stage0_weight(brov_solver* s, const double* W0) {
    invalidate_preparation(s);
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    s->has_W0 = false;
    if (W0) {
        bool same = true;
        for (int j = 0; j < 16; j++) {
            if (!(W0[j] >= 0.0) || !(W0[j] < 1e300) || (j >= 12 && !(W0[j] > 0.0))) { g_err = "brov_set_stage0_weight: weights must be finite, >= 0 (inputs > 0)"; return BROV_ERR_ARG; }
            same = same && W0[j] == s->opts.W[j];
        }
        if (!same) { std::memcpy(s->W0_host, W0, 16 * sizeof(double)); s->has_W0 = true; }
    }
    return upload_cst(s);
}
extern "C" int brov_general_grid(const brov_solver* s) { return s ? (general_grid(s) ? 1 : 0) : BROV_ERR_ARG; }

// ---- 6-disturbance model variant ----------------------------------------------------------------
__global__ void split_p18_kernel(const double* __restrict__ p18, double* __restrict__ par, double* __restrict__ rp, size_t rows, int N1, int per_stage) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (instance, stage)
    if (t >= rows) return;
    const double* src = p18 + (per_stage ? t : t / N1) * 18;
    double* p = par + t * 16;
    p[0] = src[0]; p[1] = src[1]; p[2] = src[2]; p[3] = src[5];
#pragma unroll
    for (int j = 0; j < 12; j++) p[4 + j] = src[6 + j];
    rp[t * 2] = src[3]; rp[t * 2 + 1] = src[4];
}
extern "C" int brov_enable_dist6(brov_solver* s, int on) {
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    if (on && !s->par_rp) {
        const size_t n = (size_t)s->B * (s->N + 1) * 2;
        int rc = s->mem.alloc(&s->par_rp, n, g_err);
        if (rc == BROV_OK) rc = s->mem.alloc(&s->plant.prp_plant, (size_t)s->B * 2, g_err);
        if (rc != BROV_OK) return rc;
        HIPCHK(hipMemset(s->par_rp, 0, n * sizeof(double)));
        HIPCHK(hipMemset(s->plant.prp_plant, 0, (size_t)s->B * 2 * sizeof(double)));
    }
    s->dist6 = on != 0;
    return BROV_OK;
}
extern "C" int brov_dist6_enabled(const brov_solver* s) { return s ? (s->dist6 ? 1 : 0) : BROV_ERR_ARG; }
static int need_dist6(brov_solver* s, const char* who) {
    if (!s) return BROV_ERR_ARG;
    if (!s->dist6) { g_err = std::string(who) + ": the 6-disturbance model variant is off (brov_enable_dist6)"; return BROV_ERR_ARG; }
    return BROV_OK;
}
static int set_rp(brov_solver* s, const double* d, int per_stage, bool host, void* st) {
    if (int rc = need_dist6(s, "brov_set_rp_disturbance")) return rc;
    if (!d) return BROV_ERR_ARG;
    return set_stage_rows(s, s->par_rp, d, 2, per_stage, host, st);
}
extern "C" int brov_set_rp_disturbance_host(brov_solver* s, const double* d, int per_stage) { return set_rp(s, d, per_stage, true, nullptr); }
extern "C" int brov_set_rp_disturbance_device(brov_solver* s, const double* d, int per_stage, void* st) { return set_rp(s, d, per_stage, false, st); }
extern "C" double* brov_rp_disturbance_device(brov_solver* s) { return (s && s->dist6) ? s->par_rp : nullptr; }
extern "C" int brov_get_rp_disturbance_host(brov_solver* s, double* d) {
    if (int rc = need_dist6(s, "brov_get_rp_disturbance_host")) return rc;
    if (!d) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(d, s->par_rp, (size_t)s->B * (s->N + 1) * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return BROV_OK;
}
extern "C" int brov_set_params18_host(brov_solver* s, const double* p18, int per_stage) {
    if (int rc = need_dist6(s, "brov_set_params18_host")) return rc;
    if (!p18) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    const size_t N1 = s->N + 1, rows = (size_t)s->B * N1, nsrc = (per_stage ? rows : (size_t)s->B) * 18;
    ScopedDeviceBuffer<double> tmp;
    HIPCHK(tmp.init(nsrc));
    HIPCHK(hipMemcpy(tmp.p, p18, nsrc * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(split_p18_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, nullptr, tmp.p, s->par, s->par_rp, rows, (int)N1, per_stage);
    HIPCHK(hipDeviceSynchronize());
    s->plant.params_changed();
    return BROV_OK;
}
extern "C" int brov_plant_set_rp_disturbance_host(brov_solver* s, const double* d) {
    if (int rc = need_dist6(s, "brov_plant_set_rp_disturbance_host")) return rc;
    if (!d) { s->plant.prp_plant_set = false; return BROV_OK; }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    HIPCHK(hipMemcpy(s->plant.prp_plant, d, (size_t)s->B * 2 * sizeof(double), hipMemcpyHostToDevice));
    s->plant.prp_plant_set = true;
    return BROV_OK;
}

extern "C" int brov_set_yref_stage_host(brov_solver* s, int inst, int stage, const double* y, int ny) {
    if (!s || !y || inst < 0 || inst >= s->B || stage < 0 || stage > s->N || ny < 1 || ny > 16) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    if (s->yref_shared) {  // materialise the shared window per instance first
        for (int b = 0; b < s->B; b++)
            HIPCHK(hipMemcpy(s->yref + (size_t)b * (s->N + 1) * 16, shared_window(s), (size_t)(s->N + 1) * 16 * sizeof(double), hipMemcpyDeviceToDevice));
        s->yref_shared = false;
        forget_traj_window(s);
    }
    HIPCHK(hipMemcpy(s->yref + ((size_t)inst * (s->N + 1) + stage) * 16, y, (size_t)ny * sizeof(double), hipMemcpyHostToDevice));
    return BROV_OK;
}

extern "C" int brov_traj_set_host(brov_solver* s, const double* traj, int rows) {
    if (!s || !traj || rows < 1) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    if (s->yref_view)     // the window in force is a view into the table that is about to go: keep a copy
        HIPCHK(hipMemcpy(s->yref_sh, s->yref_view, (size_t)(s->N + 1) * 16 * sizeof(double), hipMemcpyDeviceToDevice));
    // whatever window is in force -- a view, or one launch_window built from the OLD table (12 columns, end padding) -- no longer names a
    // line of the table that is coming: brov_solve_ticks(row_stride > 0) must not walk the new table from the old one's line
    forget_traj_window(s);
    if (s->traj) { hipFree(s->traj); s->traj = nullptr; }
    HIPCHK(hipMalloc((void**)&s->traj, (size_t)rows * 16 * sizeof(double)));
    HIPCHK(hipMemcpy(s->traj, traj, (size_t)rows * 16 * sizeof(double), hipMemcpyHostToDevice));
    s->traj_rows = rows;
    return BROV_OK;
}
extern "C" int brov_traj_rows(const brov_solver* s) { return s ? s->traj_rows : 0; }
extern "C" int brov_set_yref_from_traj(brov_solver* s, int line, int ncols, void* stream) {
    if (!s || !s->traj || (ncols != 12 && ncols != 16)) { g_err = "brov_set_yref_from_traj: no trajectory or bad ncols"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(s->device));
    if (int rc = order_behind_last(s, (hipStream_t)stream)) return rc;
    if (ncols == 16 && line >= 0 && line + s->N <= s->traj_rows - 1) {
        // the window is N+1 consecutive whole rows of the resident table: use them where they lie (no kernel, no copy)
        s->yref_view = s->traj + (size_t)line * 16;
    } else {
        s->yref_view = nullptr;
        launch_window(s->traj, s->traj_rows, nullptr, line, 1, s->N, ncols, s->yref_sh, (hipStream_t)stream);
    }
    s->traj_line = line; s->traj_ncols = ncols;
    s->yref_shared = true;
    HIPCHK(hipGetLastError());
    return BROV_OK;
}
extern "C" int brov_set_yref_from_traj_lines_host(brov_solver* s, const int32_t* lines, int ncols) {
    if (!s || !s->traj || !lines || (ncols != 12 && ncols != 16)) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    HIPCHK(hipMemcpy(s->lines, lines, (size_t)s->B * sizeof(int), hipMemcpyHostToDevice));
    launch_window(s->traj, s->traj_rows, s->lines, 0, s->B, s->N, ncols, s->yref, nullptr);
    s->yref_shared = false;
    forget_traj_window(s);
    HIPCHK(hipGetLastError());
    return BROV_OK;
}
extern "C" int brov_set_candidate_params_host(brov_solver* s, int kind, const double* p0, const double* p1, const double* phase) {
    if (!s || !p0 || !p1 || !phase || kind < 0 || kind > 1) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    const size_t nb = (size_t)s->B * sizeof(double);
    HIPCHK(hipMemcpy(s->scratch3, p0, nb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->scratch3 + s->B, p1, nb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->scratch3 + 2 * (size_t)s->B, phase, nb, hipMemcpyHostToDevice));
    s->cand_set = true;
    s->cand_kind = kind;
    return BROV_OK;
}
extern "C" int brov_set_yref_candidates(brov_solver* s, double t0, double dt, void* stream) {
    if (!s || !s->cand_set) { g_err = "brov_set_yref_candidates: no candidate parameters (brov_set_candidate_params_host)"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(s->device));
    if (int rc = order_behind_last(s, (hipStream_t)stream)) return rc;
    launch_candidates(s->cand_kind, s->scratch3, s->scratch3 + s->B, s->scratch3 + 2 * (size_t)s->B, t0, dt, s->B, s->N, s->yref,
                      (hipStream_t)stream);
    s->yref_shared = false;
    forget_traj_window(s);
    HIPCHK(hipGetLastError());
    return BROV_OK;
}
extern "C" int brov_set_yref_candidates_host(brov_solver* s, int kind, const double* p0, const double* p1, const double* phase,
                                             double t0, double dt) {
    const int rc = brov_set_candidate_params_host(s, kind, p0, p1, phase);
    return rc != BROV_OK ? rc : brov_set_yref_candidates(s, t0, dt, nullptr);
}
extern "C" int brov_get_yref_host(brov_solver* s, double* yref) {
    if (!s || !yref) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t per = (size_t)(s->N + 1) * 16;
    if (s->yref_shared) {
        for (int b = 0; b < s->B; b++) HIPCHK(hipMemcpy(yref + (size_t)b * per, shared_window(s), per * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        HIPCHK(hipMemcpy(yref, s->yref, per * s->B * sizeof(double), hipMemcpyDeviceToHost));
    }
    return BROV_OK;
}
// model parameters currently in force, [B][N+1][16]
extern "C" int brov_get_params_host(brov_solver* s, double* par) {
    if (!s || !par) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(par, s->par, (size_t)s->B * (s->N + 1) * 16 * sizeof(double), hipMemcpyDeviceToHost));
    return BROV_OK;
}

__global__ void copy_stage0_par_kernel(const double* __restrict__ par, double* __restrict__ pp, int B, int N1) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < B * 16) pp[t] = par[(size_t)(t >> 4) * N1 * 16 + (t & 15)];
}
__global__ void gather_status_kernel(const brov_result* __restrict__ res, int* __restrict__ out, int B) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < B) out[t] = res[t].status;
}
extern "C" int brov_plant_set_params_host(brov_solver* s, const double* p) {
    if (!s || !p) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipMemcpy(s->plant.pplant, p, (size_t)s->B * 16 * sizeof(double), hipMemcpyHostToDevice));
    s->plant.pplant_set = true;
    return BROV_OK;
}
// ---- time-varying world-frame wrench of the plant (plant_wrench.hip): thin forwards to the one host side, wrench_source.hpp -------------------
static int no_solver(const char* who) { g_err = std::string(who) + ": null argument"; return BROV_ERR_ARG; }
extern "C" int brov_plant_wrench_constant_host(brov_solver* s, const double* w) {
    return s ? s->plant.wr.constant_host(w, call_ctx(s, "brov_plant_wrench_constant_host")) : no_solver("brov_plant_wrench_constant_host");
}
extern "C" int brov_plant_wrench_periodic(brov_solver* s, uint64_t seed, double scale, double phase0, double dphi, double tz_div) {
    if (!s) return no_solver("brov_plant_wrench_periodic");
    return s->plant.wr.periodic(seed, scale, phase0, dphi, tz_div, call_ctx(s, "brov_plant_wrench_periodic"));
}
extern "C" int brov_plant_wrench_table_host(brov_solver* s, const double* tab, int rows, const double* gain) {
    return s ? s->plant.wr.table_host(tab, rows, gain, call_ctx(s, "brov_plant_wrench_table_host")) : no_solver("brov_plant_wrench_table_host");
}
extern "C" int brov_plant_wrench_off(brov_solver* s) { return s ? s->plant.wr.set_off() : no_solver("brov_plant_wrench_off"); }
extern "C" int brov_plant_wrench_mode(const brov_solver* s) { return s ? s->plant.wr.mode() : BROV_WRENCH_OFF; }
extern "C" int brov_plant_wrench_seek(brov_solver* s, int64_t tick) {
    return s ? s->plant.wr.seek(tick, call_ctx(s, "brov_plant_wrench_seek")) : no_solver("brov_plant_wrench_seek");
}
extern "C" int64_t brov_plant_wrench_tick(const brov_solver* s) { return s ? (int64_t)s->plant.wr.tick : 0; }
extern "C" int brov_plant_wrench_eval_host(brov_solver* s, int64_t tick, double* w) {
    return s ? s->plant.wr.eval_host(tick, w, s->last_stream, call_ctx(s, "brov_plant_wrench_eval_host")) : no_solver("brov_plant_wrench_eval_host");
}
// ---- thruster stage of the plant (plant_wrench.hip): thin forwards to its host side, thruster_source.hpp ----------------------------------
extern "C" void brov_thruster_default_matrix(double K[36]) { if (K) ThrusterSource::default_matrix(K); }
extern "C" int brov_thruster_set_host(brov_solver* s, const double* K, const double* lo, const double* hi, const double* gain, const double* bias,
                                      const int64_t* onset) {
    if (!s) return no_solver("brov_thruster_set_host");
    return s->plant.th.set_host(K, lo, hi, gain, bias, onset, call_ctx(s, "brov_thruster_set_host"));
}
extern "C" int brov_thruster_off(brov_solver* s) { return s ? s->plant.th.set_off() : no_solver("brov_thruster_off"); }
extern "C" int brov_thruster_enabled(const brov_solver* s) { return s && s->plant.th.on ? 1 : 0; }
extern "C" int brov_thruster_eval_host(brov_solver* s, int64_t tick, const double* commanded, double* applied, double* wrench) {
    if (!s) return no_solver("brov_thruster_eval_host");
    return s->plant.th.eval_host(tick, commanded, applied, wrench, s->last_stream, call_ctx(s, "brov_thruster_eval_host"));
}
extern "C" int brov_thruster_last_host(brov_solver* s, double* applied) {
    return s ? s->plant.th.last_host(applied, call_ctx(s, "brov_thruster_last_host")) : no_solver("brov_thruster_last_host");
}
extern "C" int brov_thruster_get_stats_host(brov_solver* s, int32_t* clip_ticks, double* lost_sq, int64_t* steps) {
    if (!s) return no_solver("brov_thruster_get_stats_host");
    return s->plant.th.get_stats_host(clip_ticks, lost_sq, steps, call_ctx(s, "brov_thruster_get_stats_host"));
}
extern "C" int brov_thruster_reset_stats(brov_solver* s) {
    return s ? s->plant.th.reset_stats(call_ctx(s, "brov_thruster_reset_stats")) : no_solver("brov_thruster_reset_stats");
}
extern "C" int brov_thruster_last_seconds(brov_solver* s, double* seconds) {
    if (!s) return no_solver("brov_thruster_last_seconds");
    HIPCHK(hipSetDevice(s->device));
    return s->plant.th.last_seconds(seconds, call_ctx(s, "brov_thruster_last_seconds"));
}
// ---- ocean current on the plant (plant_current.hip): thin forwards to its host side, current_source.hpp ----------------------------------------
extern "C" int brov_current_constant_host(brov_solver* s, const double* v) {
    return s ? s->plant.cu.constant_host(v, call_ctx(s, "brov_current_constant_host")) : no_solver("brov_current_constant_host");
}
extern "C" int brov_current_table_host(brov_solver* s, const double* tab, int rows, const double* gain) {
    return s ? s->plant.cu.table_host(tab, rows, gain, call_ctx(s, "brov_current_table_host")) : no_solver("brov_current_table_host");
}
extern "C" int brov_current_gauss_markov_host(brov_solver* s, uint64_t seed, const double* mean, const double* mu, const double* amp, const double* lo,
                                              const double* hi, double step) {
    if (!s) return no_solver("brov_current_gauss_markov_host");
    return s->plant.cu.gauss_markov_host(seed, mean, mu, amp, lo, hi, step, call_ctx(s, "brov_current_gauss_markov_host"));
}
extern "C" int brov_current_off(brov_solver* s) { return s ? s->plant.cu.set_off() : no_solver("brov_current_off"); }
extern "C" int brov_current_mode(const brov_solver* s) { return s ? s->plant.cu.mode() : BROV_CURRENT_OFF; }
extern "C" int brov_current_eval_host(brov_solver* s, int64_t tick, double* v) {
    return s ? s->plant.cu.eval_host(tick, v, s->last_stream, call_ctx(s, "brov_current_eval_host")) : no_solver("brov_current_eval_host");
}
extern "C" int brov_current_get_state_host(brov_solver* s, double* v) {
    if (!s) return no_solver("brov_current_get_state_host");
    return s->plant.cu.get_state_host(s->plant.tick(), v, s->last_stream, call_ctx(s, "brov_current_get_state_host"));
}
extern "C" int brov_current_set_state_host(brov_solver* s, const double* v) {
    return s ? s->plant.cu.set_state_host(v, call_ctx(s, "brov_current_set_state_host")) : no_solver("brov_current_set_state_host");
}
extern "C" int brov_current_last_host(brov_solver* s, double* v) {
    return s ? s->plant.cu.last_host(v, call_ctx(s, "brov_current_last_host")) : no_solver("brov_current_last_host");
}
extern "C" int brov_current_last_seconds(brov_solver* s, double* seconds) {
    if (!s) return no_solver("brov_current_last_seconds");
    HIPCHK(hipSetDevice(s->device));
    return s->plant.cu.last_seconds(seconds, call_ctx(s, "brov_current_last_seconds"));
}
// ---- Coriolis stage of the plant (plant_coriolis.hip): thin forwards to its host side, coriolis_source.hpp ------------------------------------
extern "C" int brov_coriolis_set(brov_solver* s, int terms, double ka, double ma) {
    return s ? s->plant.co.set(terms, ka, ma, call_ctx(s, "brov_coriolis_set")) : no_solver("brov_coriolis_set");
}
extern "C" int brov_coriolis_off(brov_solver* s) { return s ? s->plant.co.set_off() : no_solver("brov_coriolis_off"); }
extern "C" int brov_coriolis_terms(const brov_solver* s) { return s ? s->plant.co.terms() : 0; }
extern "C" int brov_coriolis_get(const brov_solver* s, int* terms, double* ka, double* ma) {
    if (!s) return no_solver("brov_coriolis_get");
    return s->plant.co.get(terms, ka, ma, call_ctx(const_cast<brov_solver*>(s), "brov_coriolis_get"));
}
extern "C" int brov_coriolis_eval_host(brov_solver* s, const double* x, const double* vc, double* c) {
    if (!s) return no_solver("brov_coriolis_eval_host");
    if (!x || !c) return call_ctx(s, "brov_coriolis_eval_host").refuse("null argument");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    s->plant.ensure_params(s->last_stream);   // the plant parameters the next step would use
    return s->plant.co.eval_host(x, vc, c, s->plant.pplant, s->last_stream, call_ctx(s, "brov_coriolis_eval_host"));
}
extern "C" int brov_coriolis_last_host(brov_solver* s, double* c) {
    return s ? s->plant.co.last_host(c, call_ctx(s, "brov_coriolis_last_host")) : no_solver("brov_coriolis_last_host");
}
extern "C" int brov_coriolis_last_seconds(brov_solver* s, double* seconds) {
    if (!s) return no_solver("brov_coriolis_last_seconds");
    HIPCHK(hipSetDevice(s->device));
    return s->plant.co.last_seconds(seconds, call_ctx(s, "brov_coriolis_last_seconds"));
}
// ---- sensor stage between plant and controller (sensor_kernel.hip): thin forwards to its host side, sensor_source.hpp, with sensor_wait ---------
static CallCtx sensor_ctx(brov_solver* s, const char* who) { return call_ctx(s, who, sensor_wait); }
extern "C" int brov_sensor_set_host(brov_solver* s, uint64_t seed, const double* sigma, const double* bias, const double* quant, const int32_t* period,
                                    const double* dropout) {
    if (!s) return no_solver("brov_sensor_set_host");
    return s->plant.sn.set_host(seed, sigma, bias, quant, period, dropout, s->x0, s->plant.tick(), s->last_stream,
                                sensor_ctx(s, "brov_sensor_set_host"));
}
extern "C" int brov_sensor_off(brov_solver* s) { return s ? s->plant.sn.set_off() : no_solver("brov_sensor_off"); }
extern "C" int brov_sensor_enabled(const brov_solver* s) { return s && s->plant.sn.on ? 1 : 0; }
extern "C" int brov_sensor_measure(brov_solver* s, void* stream) {
    if (!s) return no_solver("brov_sensor_measure");
    if (!s->plant.sn.on) { g_err = "brov_sensor_measure: the sensor stage is off (brov_sensor_set_host)"; return BROV_ERR_ARG; }
    if (int rc = s->plant.rewrite_ok(sensor_ctx(s, "brov_sensor_measure"))) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = order_behind_last(s, (hipStream_t)stream)) return rc;
    s->plant.rewritten((hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return BROV_OK;
}
extern "C" int brov_sensor_eval_host(brov_solver* s, int64_t index, const double* x, double* y, int32_t* dropped) {
    if (!s) return no_solver("brov_sensor_eval_host");
    return s->plant.sn.eval_host(index, x, y, dropped, s->last_stream, sensor_ctx(s, "brov_sensor_eval_host"));
}
extern "C" int brov_sensor_get_measurement_host(brov_solver* s, double* y) {
    return s ? s->plant.sn.get_measurement_host(y, sensor_ctx(s, "brov_sensor_get_measurement_host")) : no_solver("brov_sensor_get_measurement_host");
}
extern "C" int brov_sensor_get_stats_host(brov_solver* s, int32_t* dropped, double* err_sq, int64_t* refreshes) {
    if (!s) return no_solver("brov_sensor_get_stats_host");
    return s->plant.sn.get_stats_host(dropped, err_sq, refreshes, sensor_ctx(s, "brov_sensor_get_stats_host"));
}
extern "C" int brov_sensor_reset_stats(brov_solver* s) {
    return s ? s->plant.sn.reset_stats(sensor_ctx(s, "brov_sensor_reset_stats")) : no_solver("brov_sensor_reset_stats");
}
extern "C" int brov_sensor_last_seconds(brov_solver* s, double* seconds) {
    if (!s) return no_solver("brov_sensor_last_seconds");
    HIPCHK(hipSetDevice(s->device));
    return s->plant.sn.last_seconds(seconds, sensor_ctx(s, "brov_sensor_last_seconds"));
}
// ---- IMU/GPS stage behind the plant (imu_kernel.hip): thin forwards to its host side, imu_source.hpp, with sensor_wait: a refresh runs on
// whatever stream a plant step was given ---------------------------------------------------------------------------------------------------
extern "C" void brov_imu_default_params(brov_imu_params* p) {
    if (p) *p = brov_imu_params{0.01, 9.81, 1, 0, 0};
}
extern "C" int brov_imu_set_host(brov_solver* s, const brov_imu_params* p, const double* sigma, const double* bias, const double* dropout) {
    if (!s) return no_solver("brov_imu_set_host");
    return s->plant.im.set_host(p, sigma, bias, dropout, s->x0, s->plant.tick(), s->last_stream, sensor_ctx(s, "brov_imu_set_host"));
}
extern "C" int brov_imu_off(brov_solver* s) { return s ? s->plant.im.set_off() : no_solver("brov_imu_off"); }
extern "C" int brov_imu_enabled(const brov_solver* s) { return s && s->plant.im.on ? 1 : 0; }
extern "C" int brov_imu_restart(brov_solver* s, void* stream) {
    if (!s) return no_solver("brov_imu_restart");
    if (!s->plant.im.on) { g_err = "brov_imu_restart: the IMU stage is off (brov_imu_set_host)"; return BROV_ERR_ARG; }
    if (int rc = ImuSource::index_ok(s->plant.tick(), sensor_ctx(s, "brov_imu_restart"))) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = order_behind_last(s, (hipStream_t)stream)) return rc;
    s->plant.im.measure(s->x0, s->plant.tick(), true, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return BROV_OK;
}
extern "C" int brov_imu_eval_host(brov_solver* s, int64_t index, const double* x, const double* v_prev, const double* gps_p_last, const int32_t* m_last,
                                  double* imu, double* gps_p, double* gps_v, double* q_meas, int32_t* fix) {
    if (!s) return no_solver("brov_imu_eval_host");
    return s->plant.im.eval_host(index, x, v_prev, gps_p_last, m_last, imu, gps_p, gps_v, q_meas, fix, s->last_stream,
                                 sensor_ctx(s, "brov_imu_eval_host"));
}
extern "C" int brov_imu_get_host(brov_solver* s, double* imu, double* gps_p, double* gps_v, double* q_meas, int32_t* fix) {
    return s ? s->plant.im.get_host(imu, gps_p, gps_v, q_meas, fix, sensor_ctx(s, "brov_imu_get_host")) : no_solver("brov_imu_get_host");
}
extern "C" int brov_imu_get_stats_host(brov_solver* s, int32_t* stats, int64_t* refreshes) {
    return s ? s->plant.im.get_stats_host(stats, refreshes, sensor_ctx(s, "brov_imu_get_stats_host")) : no_solver("brov_imu_get_stats_host");
}
extern "C" int brov_imu_reset_stats(brov_solver* s) {
    return s ? s->plant.im.reset_stats(sensor_ctx(s, "brov_imu_reset_stats")) : no_solver("brov_imu_reset_stats");
}
extern "C" int brov_imu_last_seconds(brov_solver* s, double* seconds) {
    if (!s) return no_solver("brov_imu_last_seconds");
    HIPCHK(hipSetDevice(s->device));
    return s->plant.im.last_seconds(seconds, sensor_ctx(s, "brov_imu_last_seconds"));
}
// ---- range stage and inspection controller (inspect_kernel.hip): thin forwards to their host side, inspect_source.hpp, with sensor_wait: a tick
// runs on whatever stream it was given ---------------------------------------------------------------------------------------------------------
extern "C" void brov_range_default_params(brov_range_params* p) {
    if (p) *p = InspectSource::default_range();
}
extern "C" double brov_range_focal(double width, double hfov) { return InspectSource::focal(width, hfov); }
extern "C" int brov_range_set_scene_host(brov_solver* s, int32_t n, const double* lo, const double* hi) {
    return s ? s->plant.in.set_scene_host(n, lo, hi, sensor_ctx(s, "brov_range_set_scene_host")) : no_solver("brov_range_set_scene_host");
}
extern "C" int brov_range_set_host(brov_solver* s, const brov_range_params* p, const double* sigma) {
    return s ? s->plant.in.set_range_host(p, sigma, sensor_ctx(s, "brov_range_set_host")) : no_solver("brov_range_set_host");
}
extern "C" int brov_range_eval_host(brov_solver* s, int64_t m, const double* x, double* range, int32_t* hits, double* rot, double* depth) {
    if (!s) return no_solver("brov_range_eval_host");
    return s->plant.in.range_eval_host(m, x, range, hits, rot, depth, s->last_stream, sensor_ctx(s, "brov_range_eval_host"));
}
extern "C" int brov_range_last_seconds(brov_solver* s, double* seconds) {
    if (!s) return no_solver("brov_range_last_seconds");
    HIPCHK(hipSetDevice(s->device));
    return s->plant.in.range_last_seconds(seconds, sensor_ctx(s, "brov_range_last_seconds"));
}
extern "C" void brov_inspect_default_params(brov_inspect_params* p) {
    if (p) *p = InspectSource::default_inspect();
}
extern "C" int brov_inspect_set_host(brov_solver* s, const brov_inspect_params* p) {
    return s ? s->plant.in.set_host(p, sensor_ctx(s, "brov_inspect_set_host")) : no_solver("brov_inspect_set_host");
}
extern "C" int brov_inspect_off(brov_solver* s) { return s ? s->plant.in.set_off() : no_solver("brov_inspect_off"); }
extern "C" int brov_inspect_enabled(const brov_solver* s) { return s && s->plant.in.on ? 1 : 0; }
extern "C" int brov_inspect_reset(brov_solver* s) {
    return s ? s->plant.in.reset(sensor_ctx(s, "brov_inspect_reset")) : no_solver("brov_inspect_reset");
}
extern "C" int brov_inspect_eval_host(brov_solver* s, const brov_inspect_state* state_in, const double* range, const double* z, const double* psi,
                                      brov_inspect_state* state_out, brov_result* rec, brov_inspect_stats* stats) {
    if (!s) return no_solver("brov_inspect_eval_host");
    return s->plant.in.eval_host(state_in, range, z, psi, state_out, rec, stats, s->last_stream, sensor_ctx(s, "brov_inspect_eval_host"));
}
extern "C" int brov_inspect_get_state_host(brov_solver* s, brov_inspect_state* state, double* range) {
    return s ? s->plant.in.get_state_host(state, range, sensor_ctx(s, "brov_inspect_get_state_host")) : no_solver("brov_inspect_get_state_host");
}
extern "C" int brov_inspect_get_stats_host(brov_solver* s, brov_inspect_stats* stats) {
    return s ? s->plant.in.get_stats_host(stats, sensor_ctx(s, "brov_inspect_get_stats_host")) : no_solver("brov_inspect_get_stats_host");
}
extern "C" int brov_inspect_reset_stats(brov_solver* s) {
    return s ? s->plant.in.reset_stats(sensor_ctx(s, "brov_inspect_reset_stats")) : no_solver("brov_inspect_reset_stats");
}
extern "C" int brov_inspect_last_seconds(brov_solver* s, double* seconds) {
    if (!s) return no_solver("brov_inspect_last_seconds");
    HIPCHK(hipSetDevice(s->device));
    return s->plant.in.last_seconds(seconds, sensor_ctx(s, "brov_inspect_last_seconds"));
}
extern "C" int brov_inspect_step(brov_solver* s, void* stream) {
    if (!s) return no_solver("brov_inspect_step");
    if (int rc = s->plant.in.steps_ok(s->plant.tick(), 1, s->plant.dl.on ? s->plant.dl.ahead() : 0, sensor_ctx(s, "brov_inspect_step"))) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = order_behind_last(s, (hipStream_t)stream)) return rc;
    s->plant.in.step(s->x0, s->plant.controller_state(), s->res, s->plant.tick(), (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return BROV_OK;
}
// ---- the triangle mesh of the range stage's scene (mesh_kernel.hip): thin forwards to its host side, mesh_source.hpp, a member of the
// inspection stage's: while a mesh is set that stage launches the mesh kernels ------------------------------------------------------------
extern "C" int brov_mesh_set_host(brov_solver* s, int64_t n, const double* tri, int32_t leaf) {
    return s ? s->plant.in.mesh.set_host(n, tri, leaf, sensor_ctx(s, "brov_mesh_set_host")) : no_solver("brov_mesh_set_host");
}
extern "C" int brov_mesh_info(brov_solver* s, brov_mesh_summary* info) {
    return s ? s->plant.in.mesh.get_info(info, sensor_ctx(s, "brov_mesh_info")) : no_solver("brov_mesh_info");
}
extern "C" int brov_mesh_eval_host(brov_solver* s, int64_t m, const double* x, double* range, int32_t* hits, double* rot, double* depth,
                                   int64_t* visits) {
    if (!s) return no_solver("brov_mesh_eval_host");
    return s->plant.in.range_eval_host(m, x, range, hits, rot, depth, s->last_stream, sensor_ctx(s, "brov_mesh_eval_host"), visits, true);
}
// ---- delay stage between the controller's commands and the plant (delay_kernel.hip): thin forwards to its host side, delay_source.hpp, with
// sensor_wait: the predictor runs on whatever stream a solve was given -----------------------------------------------------------------------
extern "C" int brov_delay_set_host(brov_solver* s, const int32_t* delay, int32_t comp, double dt_pred, int32_t observer_applied) {
    if (!s) return no_solver("brov_delay_set_host");
    return s->plant.dl.set_host(delay, comp, dt_pred, s->opts.Ts, observer_applied, sensor_ctx(s, "brov_delay_set_host"));
}
extern "C" int brov_delay_off(brov_solver* s) { return s ? s->plant.dl.set_off() : no_solver("brov_delay_off"); }
extern "C" int brov_delay_enabled(const brov_solver* s) { return s && s->plant.dl.on ? 1 : 0; }
extern "C" int brov_delay_comp(const brov_solver* s) { return s ? s->plant.dl.ahead() : 0; }
extern "C" int brov_delay_depth(const brov_solver* s) { return s ? s->plant.dl.D : 0; }
extern "C" int brov_delay_reset(brov_solver* s) { return s ? s->plant.dl.reset(sensor_ctx(s, "brov_delay_reset")) : no_solver("brov_delay_reset"); }
extern "C" int brov_delay_last_host(brov_solver* s, double* u0_applied, double* thrust_applied) {
    if (!s) return no_solver("brov_delay_last_host");
    return s->plant.dl.last_host(u0_applied, thrust_applied, sensor_ctx(s, "brov_delay_last_host"));
}
extern "C" int brov_delay_queue_host(brov_solver* s, double* u0) {
    return s ? s->plant.dl.queue_host(u0, sensor_ctx(s, "brov_delay_queue_host")) : no_solver("brov_delay_queue_host");
}
extern "C" int brov_delay_predict_host(brov_solver* s, const double* y, double* xhat) {
    if (!s) return no_solver("brov_delay_predict_host");
    return s->plant.dl.predict_host(y, xhat, s->plant.controller_state(), s->plant.predict_model(), s->last_stream,
                                    sensor_ctx(s, "brov_delay_predict_host"));
}
extern "C" int brov_delay_predicted_host(brov_solver* s, double* xhat) {
    return s ? s->plant.dl.predicted_host(xhat, sensor_ctx(s, "brov_delay_predicted_host")) : no_solver("brov_delay_predicted_host");
}
extern "C" int brov_delay_last_seconds(brov_solver* s, double* shift_s, double* predict_s) {
    if (!s) return no_solver("brov_delay_last_seconds");
    HIPCHK(hipSetDevice(s->device));
    return s->plant.dl.last_seconds(shift_s, predict_s, sensor_ctx(s, "brov_delay_last_seconds"));
}
// ---- rotor stage between the delay and the thruster stage (rotor_kernel.hip): thin forwards to its host side, rotor_source.hpp, with
// sensor_wait: a shift runs on whatever stream a plant step was given ----------------------------------------------------------------------------
extern "C" int brov_rotor_coeffs(double tau, double h, double* alpha, double* beta) { return RotorSource::coeffs(tau, h, alpha, beta); }
extern "C" int brov_rotor_set_host(brov_solver* s, const double* tau, double h, const double* cmd_lo, const double* cmd_hi, int32_t observer_applied) {
    if (!s) return no_solver("brov_rotor_set_host");
    return s->plant.ro.set_host(tau, h, s->opts.Ts, cmd_lo, cmd_hi, observer_applied, sensor_ctx(s, "brov_rotor_set_host"));
}
extern "C" int brov_rotor_off(brov_solver* s) { return s ? s->plant.ro.set_off() : no_solver("brov_rotor_off"); }
extern "C" int brov_rotor_enabled(const brov_solver* s) { return s && s->plant.ro.on ? 1 : 0; }
extern "C" int brov_rotor_reset(brov_solver* s) { return s ? s->plant.ro.reset(sensor_ctx(s, "brov_rotor_reset")) : no_solver("brov_rotor_reset"); }
extern "C" int brov_rotor_set_state_host(brov_solver* s, const double* r) {
    return s ? s->plant.ro.set_state_host(r, sensor_ctx(s, "brov_rotor_set_state_host")) : no_solver("brov_rotor_set_state_host");
}
extern "C" int brov_rotor_get_state_host(brov_solver* s, double* r) {
    return s ? s->plant.ro.get_state_host(r, sensor_ctx(s, "brov_rotor_get_state_host")) : no_solver("brov_rotor_get_state_host");
}
extern "C" int brov_rotor_last_host(brov_solver* s, double* u0_applied, double* thrust_applied) {
    if (!s) return no_solver("brov_rotor_last_host");
    return s->plant.ro.last_host(u0_applied, thrust_applied, sensor_ctx(s, "brov_rotor_last_host"));
}
extern "C" int brov_rotor_get_stats_host(brov_solver* s, double* lag_sq, int64_t* steps) {
    return s ? s->plant.ro.get_stats_host(lag_sq, steps, sensor_ctx(s, "brov_rotor_get_stats_host")) : no_solver("brov_rotor_get_stats_host");
}
extern "C" int brov_rotor_get_coeffs_host(brov_solver* s, double* alpha, double* beta, double* h) {
    if (!s) return no_solver("brov_rotor_get_coeffs_host");
    return s->plant.ro.get_coeffs_host(alpha, beta, h, sensor_ctx(s, "brov_rotor_get_coeffs_host"));
}
extern "C" int brov_rotor_eval_host(brov_solver* s, const double* commanded, const double* state, double* applied, double* state_out) {
    if (!s) return no_solver("brov_rotor_eval_host");
    return s->plant.ro.eval_host(commanded, state, applied, state_out, s->last_stream, sensor_ctx(s, "brov_rotor_eval_host"));
}
extern "C" int brov_rotor_last_seconds(brov_solver* s, double* seconds) {
    if (!s) return no_solver("brov_rotor_last_seconds");
    HIPCHK(hipSetDevice(s->device));
    return s->plant.ro.last_seconds(seconds, sensor_ctx(s, "brov_rotor_last_seconds"));
}
// ---- thrust-curve stage around the rotor stage (curve_kernel.hip): thin forwards to its host side, curve_source.hpp, with sensor_wait ---------
extern "C" void brov_curve_default_params(brov_curve_params* p) { CurveSource::default_params(p); }
extern "C" int brov_curve_set_table_host(brov_solver* s, int32_t which, const double* x, const double* y, const double* amps, int32_t K) {
    if (!s) return no_solver("brov_curve_set_table_host");
    return s->plant.cv.set_table_host(which, x, y, amps, K, sensor_ctx(s, "brov_curve_set_table_host"));
}
extern "C" int brov_curve_get_table_host(brov_solver* s, int32_t which, double* x, double* y, double* slope, double* amps, double* amps_slope,
                                         int32_t* K) {
    if (!s) return no_solver("brov_curve_get_table_host");
    return s->plant.cv.get_table_host(which, x, y, slope, amps, amps_slope, K, sensor_ctx(s, "brov_curve_get_table_host"));
}
extern "C" int brov_curve_set_host(brov_solver* s, const brov_curve_params* p, const double* eff) {
    return s ? s->plant.cv.set_host(p, eff, sensor_ctx(s, "brov_curve_set_host")) : no_solver("brov_curve_set_host");
}
extern "C" int brov_curve_off(brov_solver* s) { return s ? s->plant.cv.set_off() : no_solver("brov_curve_off"); }
extern "C" int brov_curve_enabled(const brov_solver* s) { return s && s->plant.cv.on ? 1 : 0; }
extern "C" int brov_curve_reset(brov_solver* s) { return s ? s->plant.cv.reset(sensor_ctx(s, "brov_curve_reset")) : no_solver("brov_curve_reset"); }
extern "C" int brov_curve_eval_host(brov_solver* s, int32_t part, const double* in, double* out, double* amps_out) {
    if (!s) return no_solver("brov_curve_eval_host");
    return s->plant.cv.eval_host(part, in, out, amps_out, s->last_stream, sensor_ctx(s, "brov_curve_eval_host"));
}
extern "C" int brov_curve_last_host(brov_solver* s, double* u0_applied, double* wanted, double* command, double* thrust) {
    if (!s) return no_solver("brov_curve_last_host");
    return s->plant.cv.last_host(u0_applied, wanted, command, thrust, sensor_ctx(s, "brov_curve_last_host"));
}
extern "C" int brov_curve_get_stats_host(brov_solver* s, double* err_sq, int32_t* dead_ticks, double* charge, int64_t* steps) {
    if (!s) return no_solver("brov_curve_get_stats_host");
    return s->plant.cv.get_stats_host(err_sq, dead_ticks, charge, steps, sensor_ctx(s, "brov_curve_get_stats_host"));
}
extern "C" int brov_curve_reset_stats(brov_solver* s) {
    return s ? s->plant.cv.reset_stats(sensor_ctx(s, "brov_curve_reset_stats")) : no_solver("brov_curve_reset_stats");
}
extern "C" int brov_curve_last_seconds(brov_solver* s, double* command_s, double* thrust_s) {
    if (!s) return no_solver("brov_curve_last_seconds");
    HIPCHK(hipSetDevice(s->device));
    return s->plant.cv.last_seconds(command_s, thrust_s, sensor_ctx(s, "brov_curve_last_seconds"));
}
// ---- the end of the forwards: from here on the plant is asked as one object ------------------------------------------------------------------
extern "C" int brov_plant_step(brov_solver* s, double dt, int substeps, void* stream) {
    if (!s || !(dt > 0.0) || substeps < 1) return BROV_ERR_ARG;
    if (int rc = s->plant.dt_ok(dt, call_ctx(s, "brov_plant_step"))) return rc;
    if (int rc = s->plant.steps_ok(1, call_ctx(s, "brov_plant_step"))) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = order_behind_last(s, (hipStream_t)stream)) return rc;
    s->plant.ensure_params((hipStream_t)stream);
    s->plant.step(dt, substeps, nullptr, nullptr, nullptr, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return BROV_OK;
}
extern "C" int brov_get_x0_host(brov_solver* s, double* x0) {
    if (!s || !x0) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(x0, s->x0, (size_t)s->B * 12 * sizeof(double), hipMemcpyDeviceToHost));
    return BROV_OK;
}
// ---- which kernels a call launches, and from which workspace: decided here, once per call ------------------------------------------------
// LDS-resident kernels serve the one-call step (rti_phase 0) on the uniform and the general grid: the fused ones the whole horizon for
// N <= 23, the windowed ones above.  rti_phase 1 / 2 (preparation and feedback as separate calls) need something to carry the preparation
// over: the streaming pair keeps the linearisation in HBM; the windowed kernel's RESIDENT configuration -- at most one instance per CU, a
// workspace per instance -- has split launches (rti_window_kernel_res_split): the preparation parks the factorised LDS image per instance,
// the feedback runs from the forward sweep on.  Fused-kernel horizons take that configuration from a workspace of its own (ws_split, see
// plan_workspaces).  A feedback call follows the path its preparation took (prep_path); BROV_SPLIT_RESIDENT=0: the streaming pair.
enum { FAM_STREAMING = 0, FAM_FUSED, FAM_WINDOWED };
struct SolvePlan {
    int family = FAM_STREAMING;
    bool split_ok = false;           // the solver's settings allow the resident split launches for rti_phase 1 / 2
    int rti_split = 0;               // windowed family: 0 one launch, 1 / 2 the resident split launch of that rti_phase
    double* ws = nullptr;            // windowed family: workspace (the solver's ws, or ws_split at a fused-kernel horizon), doubles per block,
    int64_t ws_stride = 0;           // ... stages per window and persistent blocks of THIS launch
    int win_L = 0, win_blocks = 0;
    int pit = 0, pit_blocks = 0;     // parallel-in-time kernel ahead of the resident one: DevParams::pit (0: not launched), its blocks
    int prep_path = 1;               // what brov_solver::prep_path becomes when this call is a preparation
};
static SolvePlan plan_solve(const brov_solver* s, int rti_phase) {
    SolvePlan p;
    const bool lds = s->opts.kernel_path != BROV_PATH_STREAMING, fused_h = serves_fused(s);
    const bool may_split = lds && !s->dump_lin && s->k.split_resident;
    const bool split_fused = may_split && fused_h && s->ws_split != nullptr;
    p.split_ok = split_fused || (may_split && !fused_h && s->ws != nullptr && windowed_is_resident(s->win_L) && s->win_blocks == s->B);
    const bool split = p.split_ok && (rti_phase == 1 || (rti_phase == 2 && s->prep_path == 2));
    p.prep_path = split ? 2 : 1;
    p.ws = s->ws; p.win_L = s->win_L; p.win_blocks = s->win_blocks;
    if (split && split_fused) { p.ws = s->ws_split; p.win_L = s->N; p.win_blocks = s->B; }   // one window = the horizon, one block per instance
    p.ws_stride = p.win_L ? (int64_t)windowed_ws_doubles(s->N, p.win_L) : 0;
    if (!lds || (rti_phase != 0 && !split)) return p;
    if (fused_h && !split) { p.family = FAM_FUSED; return p; }
    if (!p.ws) return p;             // (a solver created with BROV_PATH_STREAMING has no workspace: the streaming pair whatever the path says now)
    p.family = FAM_WINDOWED;
    p.rti_split = rti_phase;
    p.pit_blocks = p.win_blocks;
    // The parallel-in-time kernel (BROV_PIT=0 off, 2: every instance is tried, not only those whose previous step was an early exit) runs whenever
    // it can serve the solve -- a constant rule since round 5: it runs the whole QP loop itself (qp/pit.hpp), so what it leaves to the resident
    // kernel behind it are the instances it gives up on (a NaN, a pivot block that fails or is ill-conditioned: verdicts of its first pass), and
    // those cost it next to nothing.
    bool pit = false;
    if (s->k.pit && rti_phase == 2) {
        // feedback of a split tick: its feedback instantiation rolls out the four quarters at once from what the preparation parked
        pit = s->k.split_parallel && pit_supported(s->N, p.win_L);
    } else if (s->k.pit && rti_phase == 0 && !s->dump_lin) {
        if (s->alt_L) {              // between one and two instances per CU: the resident configuration, one rti_pit_kernel block per instance
            p.win_L = s->alt_L; p.win_blocks = s->alt_blocks; p.ws_stride = (int64_t)windowed_ws_doubles(s->N, s->alt_L);
            p.pit_blocks = s->B;
        }
        pit = pit_supported(s->N, p.win_L);
    }
    p.pit = pit ? s->k.pit : 0;
    return p;
}

static DevParams make_params(const brov_solver* s, const SolvePlan& plan, const LaunchInputs* in = nullptr) {
    static const LaunchInputs none;
    if (!in) in = &none;
    DevParams P;
    std::memset(&P, 0, sizeof P);
    P.B = s->B; P.N = s->N;
    P.qp_iter_max = s->opts.qp_iter_max; P.early_exit = s->opts.qp_early_exit;
    P.on_failure = s->opts.on_failure; P.dump_lin = s->dump_lin ? 1 : 0;
    P.robust_kkt_max = s->k.robust_kkt_max;
    P.robust_pivot = s->k.robust_pivot;            // development knob: 0 off, 1 on demand (default), 2 every instance
    P.partial_refactor = s->k.partial_refactor;    // development knob (A/B, tests)
    P.Ts = s->opts.Ts; P.tol_mu = s->opts.qp_tol_mu; P.tol_stat = s->opts.qp_tol_stat;
    for (int j = 0; j < 16; j++) P.W[j] = s->opts.W[j];
    for (int j = 0; j < 12; j++) P.We[j] = s->opts.We[j];
    for (int j = 0; j < 4; j++) { P.lbu[j] = s->opts.lbu[j]; P.ubu[j] = s->opts.ubu[j]; }
    // sensor stage on: the measured state; a tick's own x0 is the caller's measurement; delay stage with comp > 0: the predictor's (predicted_inputs)
    P.x0 = in->x0 ? in->x0 : s->plant.controller_state();
    P.yref = in->yref ? in->yref : (s->yref_shared ? shared_window(s) : s->yref);
    P.yref_stride = s->yref_shared ? 0 : (int64_t)(s->N + 1) * 16;
    P.par = in->par ? in->par : s->par;
    P.par_rp = s->dist6 ? s->par_rp : nullptr;
    P.tsv = general_grid(s) ? s->tsv : nullptr;
    P.sched = s->k.sched ? s->sched : nullptr;   // development knob: BROV_SCHED=0 hands the instances out in index order (A/B of the work ordering)
    P.sched_stride = sched_buffer_ints_host(s->B);
    P.sched_r = (int)(s->sched_tick % 3); P.sched_w = (int)((s->sched_tick + 1) % 3); P.sched_z = (int)((s->sched_tick + 2) % 3);
    P.wst = general_grid(s) ? s->wst : nullptr;
    P.x = s->x; P.u = s->u; P.pi = s->pi; P.lam = s->lam;
    P.BA = s->BA; P.bvec = s->bvec; P.kktp = s->kktp;
    P.Ks = s->Ks; P.Kt = s->Kt; P.Mt = s->Mt; P.Pb = s->Pb; P.kff = s->kff; P.vhat = s->vhat; P.ipm = s->ipm;
    P.dxb = s->dxb; P.cst = s->cst; P.res = s->res;
    P.mail = in->mail; P.mail_flag = in->mail_flag; P.mail_seq = in->mail_seq;
    P.mail_early = s->k.mail_early;   // development knob (A/B)
    P.counter = s->counter + 32 * (s->win_count & 1u);
    P.counter_next = s->counter + 32 * ((s->win_count + 1u) & 1u);
    P.ws = plan.ws; P.ws_stride = plan.ws_stride; P.win_L = plan.win_L; P.win_blocks = plan.win_blocks;
    P.rti_split = plan.rti_split; P.pit_blocks = plan.pit_blocks;
    if (plan.pit) { P.pit = plan.pit; P.pit_done = s->pit_done; P.pit_try = s->k.pit_try; P.pit_light = s->k.pit_light; }
    P.dbg = s->dbg;
    return P;
}
// Delay stage with comp > 0: the solve starts comp plant steps ahead.  The predictor runs on `st` ahead of the launch (the caller has ordered
// `st`) and the launch reads its x0 from the predictor's buffer: make_params takes it as it takes a tick's own x0.  Parameters passed with a
// tick are the predictor's too.  Returns what make_params is given: `in`, or `with`, a copy of it with the predicted state as x0.
static const LaunchInputs* predicted_inputs(brov_solver* s, const LaunchInputs* in, LaunchInputs& with, hipStream_t st) {
    if (!s->plant.dl.predicts() || (in && in->x0)) return in;
    if (in) with = *in;
    with.x0 = s->plant.predict(in ? in->par : nullptr, st);
    return &with;
}
// the launch(es) of an LDS-resident family and what the solver remembers of them
static void launch_lds(brov_solver* s, const DevParams& P, int family, hipStream_t st) {
    if (family == FAM_FUSED) launch_fused(P, st, s->k);
    else { launch_windowed(P, st, s->k); s->win_count++; }   // persistent blocks; the two hand-out counters alternate
    s->pit_ran = P.pit != 0;
    s->last_family = family;
    s->last_stream = st;
}
// brov_enable_timing: event k of the three around a solve's launches (0 start, 1 linearisation done / the one launch starts, 2 end), which
// brov_last_solve_seconds reads
static void time_mark(brov_solver* s, int k, hipStream_t st) {
    if (s->timing) { hipEventRecord(s->ev[k], st); s->ev_valid = s->ev_valid || k == 2; }
}
// `n` steps of every instance in ONE launch of the family's *_ticks kernel on `st`, the shared window moving on row_stride_doubles per step;
// the window in force afterwards is the last step's.  brov_last_solve_seconds then reports THIS launch.
static int launch_ticks(brov_solver* s, int family, int n, int64_t row_stride_doubles, int32_t* status_log, const PlantInLaunch* plant,
                        hipStream_t st) {
    if (int rc = order_behind_last(s, st)) return rc;
    LaunchInputs pred;   // (delay stage: every step of the launch starts from the one prediction; a plant in the launch is plain, so there is none)
    DevParams P = make_params(s, plan_solve(s, 0), predicted_inputs(s, nullptr, pred, st));
    P.sched = nullptr;                // a launch of many steps neither reads nor writes the work ordering: every instance follows its own history
    P.ticks = n; P.tick_yref = row_stride_doubles; P.tick_status = status_log;
    if (plant) s->plant.into_ticks(P, *plant);   // (moves the plant's counter on by the n steps)
    time_mark(s, 0, st); time_mark(s, 1, st);
    launch_lds(s, P, family, st); s->prep_path = 0;
    time_mark(s, 2, st);
    if (row_stride_doubles > 0) {
        s->traj_line += (n - 1) * (int)(row_stride_doubles / 16);
        s->yref_view = s->traj + (size_t)s->traj_line * 16;
    }
    return BROV_OK;
}

static int ticks_kernel(const brov_solver* s);
// The columns of the solver's loop logs (LoopLog, host_common.hpp), entry j = tick j of the run: the plant state AFTER the tick, the applied
// input, the status, the applied wrench, the observer's estimate.  A whole loop (brov_closed_loop_ex / _dob) has a column per HOST log the
// caller asked for, the states behind the start state; a chunk of brov_closed_loop_track has x, u and status on the device alone.
enum { LOG_X, LOG_U, LOG_ST, LOG_W, LOG_EST };
static void declare_logs(LoopLog& L, double* x, double* u, int32_t* st, double* w, double* est, bool chunk) {
    L.column(12, x, chunk ? 0 : 1, chunk); L.column(4, u, 0, chunk); L.column(1, st, 0, chunk); L.column(6, w); L.column(6, est);
}
// a whole loop's logs on `st`: allocated, the start state ahead of the states, and the wrench log zeroed where no wrench kernel writes it
static int begin_logs(LoopLog& L, const brov_solver* s, int ticks, hipStream_t st, const std::string& pre) {
    if (int rc = L.alloc(s->B, ticks, g_err, pre)) return rc;
    return L.init(s->x0, brov_plant_wrench_mode(s) == BROV_WRENCH_OFF ? LOG_W : -1, st, g_err, pre);
}
// what the closed-loop entry points ask of their arguments alike, reported under the caller's name (an observer and an estimator are optional
// here; brov_closed_loop_dob asks for its observer itself)
static int loop_args_ok(brov_solver* s, const brov_ekf* e, const brov_rls* r, int rls_mode, int ticks, int ncols, double dt, int substeps,
                        const char* who) {
    if (!s || (r && !e) || ticks < 1 || !s->traj || (ncols != 12 && ncols != 16) || !(dt > 0.0) || substeps < 1) {
        g_err = std::string(who) + ": bad argument (needs ticks >= 1, ncols 12 or 16, dt > 0, substeps >= 1, an observer with an estimator, and a "
                                   "trajectory table, see brov_traj_set_host)";
        return BROV_ERR_ARG;
    }
    if ((e && brov_ekf_batch(e) != s->B) || (r && brov_rls_batch(r) != s->B)) { g_err = std::string(who) + ": batch sizes differ"; return BROV_ERR_ARG; }
    if (r && rls_mode != BROV_RLS_APPLY_DISTURBANCE && rls_mode != BROV_RLS_APPLY_MODEL) { g_err = std::string(who) + ": unknown rls_mode"; return BROV_ERR_ARG; }
    if (int rc = s->plant.dt_ok(dt, call_ctx(s, who))) return rc;
    return s->plant.steps_ok(ticks, call_ctx(s, who));
}
// the statuses of the step just enqueued on `st` into a DEVICE log row (null: not logged)
static void gather_status(const brov_solver* s, int* out, hipStream_t st) {
    if (out) hipLaunchKernelGGL(gather_status_kernel, dim3((unsigned)((s->B + 255) / 256)), dim3(256), 0, st, s->res, out, (int)s->B);
}
// whether brov_closed_loop_ex runs `ticks` ticks from `line0` as one launch, and with which kernel.
// One launch for the whole loop where the fused kernels serve the solver and every window is rows of the table in place (round 5,
// rti_fused_kernel_ticks with the plant update behind every step): every instance runs its own closed loop at its own pace -- no launch
// boundaries, three launches per tick saved, and a tick on which one instance grinds through the QP loop holds nobody else.
// (The fused and windowed *_ticks kernels integrate the plant themselves and know none of its stages: unless the plant is plain, the loop
// takes a launch per step.)
static bool loop_in_one_launch(const brov_solver* s, int ticks, int line0, int ncols, int* which) {
    *which = ticks_kernel(s);
    return s->k.closed_loop_fused && ncols == 16 && line0 >= 0 && line0 + (ticks - 1) + s->N <= s->traj_rows - 1 && *which != 0 &&
           s->plant.plain();
}
// `n` ticks of the plain loop (window -> RTI step -> plant step) from trajectory row `line` on `st`, logged into L
static int run_loop_ticks(brov_solver* s, int n, int line, int ncols, double dt, int substeps, bool one_launch, int which, const LoopLog& L,
                          hipStream_t st) {
    int rc = BROV_OK;
    if (one_launch) {
        rc = brov_set_yref_from_traj(s, line, 16, st);
        const PlantInLaunch plant{dt, substeps, L.row<double>(LOG_X, 0), L.row<double>(LOG_U, 0)};
        if (rc == BROV_OK) rc = launch_ticks(s, which, n, 16, L.row<int32_t>(LOG_ST, 0), &plant, st);
    }
    const int ahead = s->plant.dl.ahead();   // delay stage: the OCP starts comp ticks ahead, and so does its window (the stage is never plain: no one_launch)
    for (int k = 0; k < n && rc == BROV_OK && !one_launch; k++) {
        forget_traj_window(s);
        launch_window(s->traj, s->traj_rows, nullptr, line + k + ahead, 1, s->N, ncols, s->yref_sh, st);
        s->yref_shared = true;
        rc = brov_solve_phase(s, st, 0);
        gather_status(s, L.row<int32_t>(LOG_ST, k), st);
        s->plant.step(dt, substeps, L.row<double>(LOG_X, k), L.row<double>(LOG_U, k), L.row<double>(LOG_W, k), st);
    }
    return rc;
}
// `n` ticks of the DOB / AMPC loop from trajectory row `line` on `st`: per tick the five public calls of the header.  The observer's and the
// estimator's calls report through their own error strings: their code is handed on, their text copied behind `who`
static int run_dob_ticks(brov_solver* s, brov_ekf* e, brov_rls* r, int rls_mode, int n, int line, int ncols, double dt, int substeps,
                         const LoopLog& L, hipStream_t st, const char* who) {
    const size_t B = s->B;
    int rc = BROV_OK;
    auto sub = [&](int code, const char* text) {
        if (code != BROV_OK) { g_err = std::string(who) + ": " + text; rc = code; }
        return code == BROV_OK;
    };
    const int ahead = s->plant.dl.ahead();   // delay stage: the OCP starts comp ticks ahead, and so does its window
    for (int k = 0; k < n && rc == BROV_OK; k++) {
        rc = brov_set_yref_from_traj(s, line + k + ahead, ncols, st);
        if (rc == BROV_OK) rc = brov_solve_phase(s, st, 0);
        if (rc != BROV_OK) break;
        gather_status(s, L.row<int32_t>(LOG_ST, k), st);
        s->plant.ensure_params(st);   // (the hand-off below rewrites the controller's stage 0, which a plant without parameters of its own follows)
        s->plant.step(dt, substeps, L.row<double>(LOG_X, k), L.row<double>(LOG_U, k), L.row<double>(LOG_W, k), st);
        if (!sub(brov_ekf_update_from_solver(e, s, st), brov_ekf_last_error())) break;
        if (double* est = L.row<double>(LOG_EST, k)) launch_gather_cols(brov_ekf_x_device(e), (int)B, 18, 12, 6, est, st);
        if (!r) sub(brov_ekf_apply_to_solver(e, s, st), brov_ekf_last_error());
        else if (sub(brov_rls_update_from_ekf(r, e, s, st), brov_rls_last_error())) sub(brov_rls_apply_to_solver(r, s, rls_mode, st), brov_rls_last_error());
    }
    return rc;
}
extern "C" int brov_closed_loop(brov_solver* s, int ticks, int line0, int ncols, double dt, int substeps, double* u_log, double* x_log,
                                int32_t* st_log) {
    return brov_closed_loop_ex(s, ticks, line0, ncols, dt, substeps, u_log, x_log, st_log, nullptr);
}
extern "C" int brov_closed_loop_ex(brov_solver* s, int ticks, int line0, int ncols, double dt, int substeps, double* u_log, double* x_log,
                                   int32_t* st_log, double* w_log) {
    if (int rc = loop_args_ok(s, nullptr, nullptr, 0, ticks, ncols, dt, substeps, "brov_closed_loop")) return rc;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = s->last_stream;
    s->plant.ensure_params(st);
    LoopLog L;
    declare_logs(L, x_log, u_log, st_log, w_log, nullptr, false);
    int rc = begin_logs(L, s, ticks, st, "brov_closed_loop: ");
    int which = 0;
    const bool one_launch = loop_in_one_launch(s, ticks, line0, ncols, &which);
    if (rc == BROV_OK) rc = run_loop_ticks(s, ticks, line0, ncols, dt, substeps, one_launch, which, L, st);
    return L.deliver(finish_loop(st, rc, g_err, ""), g_err, "brov_closed_loop: ");
}

// The DOB / AMPC loop on the device: per tick the five public calls of the header, on one stream, one host wait at the end.
extern "C" int brov_closed_loop_dob(brov_solver* s, brov_ekf* e, brov_rls* r, int rls_mode, int ticks, int line0, int ncols, double dt, int substeps,
                                    double* u_log, double* x_log, int32_t* st_log, double* w_log, double* est_log) {
    if (!e) { g_err = "brov_closed_loop_dob: bad argument (needs an observer)"; return BROV_ERR_ARG; }
    if (int rc = loop_args_ok(s, e, r, rls_mode, ticks, ncols, dt, substeps, "brov_closed_loop_dob")) return rc;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = s->last_stream;
    LoopLog L;
    declare_logs(L, x_log, u_log, st_log, w_log, est_log, false);
    int rc = begin_logs(L, s, ticks, st, "brov_closed_loop_dob: ");
    if (rc == BROV_OK) rc = run_dob_ticks(s, e, r, rls_mode, ticks, line0, ncols, dt, substeps, L, st, "brov_closed_loop_dob");
    return L.deliver(finish_loop(st, rc, g_err, ""), g_err, "brov_closed_loop_dob: ");
}

// The loop with the error-state filter at its sensors' rates: per control tick the public calls of the header (bluerov2_nmpc_imu.h), on one
// stream, one host wait at the end.  The logs' columns are those of declare_logs, the estimate three wide, and the fix flags behind them
extern "C" int brov_closed_loop_eskf(brov_solver* s, brov_eskf* e, int ticks, int line0, int ncols, double dt, int imu_per_tick, double* u_log,
                                     double* x_log, int32_t* st_log, double* w_log, double* est_log, int32_t* fix_log) {
    const char* who = "brov_closed_loop_eskf";
    if (!e) { g_err = "brov_closed_loop_eskf: bad argument (needs an observer)"; return BROV_ERR_ARG; }
    if (imu_per_tick < 1) { g_err = "brov_closed_loop_eskf: bad argument (needs imu_per_tick >= 1)"; return BROV_ERR_ARG; }
    const double h = dt / imu_per_tick;   // the plant steps of the loop: what the stages in force are asked about
    if (int rc = loop_args_ok(s, nullptr, nullptr, 0, ticks, ncols, h, 1, who)) return rc;
    if (brov_eskf_batch(e) != s->B) { g_err = "brov_closed_loop_eskf: batch sizes differ"; return BROV_ERR_ARG; }
    if (!s->plant.im.on) { g_err = "brov_closed_loop_eskf: the IMU stage of the solver is off (brov_imu_set_host)"; return BROV_ERR_ARG; }
    if (int rc = s->plant.steps_ok((long long)ticks * imu_per_tick, call_ctx(s, who))) return rc;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = s->last_stream;
    LoopLog L;
    L.column(12, x_log, 1); L.column(4, u_log); L.column(1, st_log); L.column(6, w_log); L.column(3, est_log);
    const int log_fix = L.column((size_t)imu_per_tick, fix_log);
    int rc = begin_logs(L, s, ticks, st, "brov_closed_loop_eskf: ");
    auto sub = [&](int code) {
        if (code != BROV_OK) { g_err = std::string(who) + ": " + brov_eskf_last_error(); rc = code; }
        return code == BROV_OK;
    };
    const size_t B = s->B;
    for (int k = 0; k < ticks && rc == BROV_OK; k++) {
        rc = brov_set_yref_from_traj(s, line0 + k, ncols, st);
        if (rc == BROV_OK) rc = brov_solve_phase(s, st, 0);
        if (rc != BROV_OK) break;
        gather_status(s, L.row<int32_t>(LOG_ST, k), st);
        for (int j = 0; j < imu_per_tick && rc == BROV_OK; j++) {
            const bool last = j == imu_per_tick - 1;   // the tick's logs are its last plant step's
            s->plant.ensure_params(st);
            s->plant.step(h, 1, last ? L.row<double>(LOG_X, k) : nullptr, last ? L.row<double>(LOG_U, k) : nullptr,
                          last ? L.row<double>(LOG_W, k) : nullptr, st);
            if (!sub(brov_imu_eskf_tick_from_solver(e, s, st))) break;
            if (int32_t* fx = L.row<int32_t>(log_fix, k))
                if (hipMemcpyAsync(fx + (size_t)j * B, s->plant.im.out.fix, B * sizeof(int32_t), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = BROV_ERR_HIP;
        }
        if (rc != BROV_OK) break;
        if (double* est = L.row<double>(LOG_EST, k))
            if (hipMemcpyAsync(est, brov_imu_eskf_xi_world_device(e), B * 3 * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = BROV_ERR_HIP;
        if (rc == BROV_OK) sub(brov_eskf_apply_to_solver(e, s, st));
    }
    return L.deliver(finish_loop(st, rc, g_err, ""), g_err, "brov_closed_loop_eskf: ");
}

// The inspection loop: per tick brov_inspect_step and brov_plant_step, on one stream, one host wait at the end.  Columns: the states behind the
// start state, the commanded input, the mission status, the range
extern "C" int brov_closed_loop_inspect(brov_solver* s, int ticks, double dt, int substeps, double* u_log, double* x_log, int32_t* st_log,
                                        double* r_log) {
    const char* who = "brov_closed_loop_inspect";
    if (!s) return no_solver(who);
    if (ticks < 1 || !(dt > 0.0) || substeps < 1) { g_err = "brov_closed_loop_inspect: bad argument (needs ticks >= 1, dt > 0, substeps >= 1)"; return BROV_ERR_ARG; }
    if (int rc = s->plant.in.steps_ok(s->plant.tick(), ticks, s->plant.dl.on ? s->plant.dl.ahead() : 0, call_ctx(s, who))) return rc;
    if (int rc = s->plant.dt_ok(dt, call_ctx(s, who))) return rc;
    if (int rc = s->plant.steps_ok(ticks, call_ctx(s, who))) return rc;
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = s->last_stream;
    LoopLog L;
    const int log_x = L.column(12, x_log, 1), log_u = L.column(4, u_log), log_st = L.column(1, st_log), log_r = L.column(1, r_log);
    int rc = L.alloc(s->B, ticks, g_err, "brov_closed_loop_inspect: ");
    if (rc == BROV_OK) rc = L.init(s->x0, -1, st, g_err, "brov_closed_loop_inspect: ");
    const InspectSource& in = s->plant.in;
    for (int k = 0; k < ticks && rc == BROV_OK; k++) {
        s->plant.in.step(s->x0, s->plant.controller_state(), s->res, s->plant.tick(), st);
        if (int32_t* row = L.row<int32_t>(log_st, k))
            if (hipMemcpyAsync(row, in.dev.status, s->B * sizeof(int32_t), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = BROV_ERR_HIP;
        if (double* row = L.row<double>(log_r, k))
            if (hipMemcpyAsync(row, in.dev.range, s->B * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = BROV_ERR_HIP;
        s->plant.ensure_params(st);
        s->plant.step(dt, substeps, L.row<double>(log_x, k), L.row<double>(log_u, k), nullptr, st);
    }
    return L.deliver(finish_loop(st, rc, g_err, ""), g_err, "brov_closed_loop_inspect: ");
}

namespace brov {
// one accumulate of the tracking statistics over DEVICE logs on `st`, saturation judged by the given bounds (track_kernel.hip)
int track_accumulate_on(brov_track* t, const double* x, const double* u, const int* status, int K, const double* ref, int rows, int line1,
                        const double* lbu, const double* ubu, hipStream_t st);
}
// The same loops scored instead of logged (brov_track_*, track_kernel.hip): chunks of ticks into DEVICE logs of one chunk, one accumulate behind
// every chunk on the same stream, one host wait at the end.
extern "C" int brov_closed_loop_track(brov_solver* s, brov_ekf* e, brov_rls* r, int rls_mode, brov_track* t, int ticks, int line0, int ncols,
                                      double dt, int substeps, int chunk) {
    if (!t || chunk < 0) { g_err = "brov_closed_loop_track: bad argument (needs a tracker and chunk >= 0)"; return BROV_ERR_ARG; }
    if (int rc = loop_args_ok(s, e, r, rls_mode, ticks, ncols, dt, substeps, "brov_closed_loop_track")) return rc;
    if (brov_track_batch(t) != s->B) { g_err = "brov_closed_loop_track: batch sizes differ"; return BROV_ERR_ARG; }
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = s->last_stream;
    if (!e) s->plant.ensure_params(st);
    int which = 0;
    const bool one_launch = !e && loop_in_one_launch(s, ticks, line0, ncols, &which);   // decided for the whole run, as brov_closed_loop_ex does
    const int C = std::min(chunk == 0 ? 64 : chunk, ticks);
    LoopLog L;   // one chunk, on the device alone
    declare_logs(L, nullptr, nullptr, nullptr, nullptr, nullptr, true);
    int rc = L.alloc(s->B, C, g_err, "brov_closed_loop_track: ");
    for (int k0 = 0; k0 < ticks && rc == BROV_OK; k0 += C) {
        const int n = std::min(C, ticks - k0);
        rc = e ? run_dob_ticks(s, e, r, rls_mode, n, line0 + k0, ncols, dt, substeps, L, st, "brov_closed_loop_track")
               : run_loop_ticks(s, n, line0 + k0, ncols, dt, substeps, one_launch, which, L, st);
        if (rc != BROV_OK) break;
        // the state after tick k against row line0 + k + 1, by the solver's bounds of the moment
        rc = track_accumulate_on(t, L.row<double>(LOG_X, 0), L.row<double>(LOG_U, 0), L.row<int32_t>(LOG_ST, 0), n, s->traj, s->traj_rows,
                                 line0 + k0 + 1, s->opts.lbu, s->opts.ubu, st);
        if (rc != BROV_OK) g_err = std::string("brov_closed_loop_track: ") + brov_track_last_error();
    }
    return finish_loop(st, rc, g_err, "");
}

extern "C" int brov_set_iterate_host(brov_solver* s, const double* x, const double* u, const double* pi, const double* lam) {
    invalidate_preparation(s);
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));   // a solve on a non-blocking stream may still be writing the iterate
    const size_t B = s->B, N = s->N;
    if (x) HIPCHK(hipMemcpy(s->x, x, B * (N + 1) * 12 * sizeof(double), hipMemcpyHostToDevice));
    if (u) HIPCHK(hipMemcpy(s->u, u, B * N * 4 * sizeof(double), hipMemcpyHostToDevice));
    if (pi) HIPCHK(hipMemcpy(s->pi, pi, B * N * 12 * sizeof(double), hipMemcpyHostToDevice));
    if (lam) HIPCHK(hipMemcpy(s->lam, lam, B * N * 8 * sizeof(double), hipMemcpyHostToDevice));
    return BROV_OK;
}
extern "C" int brov_get_iterate_host(brov_solver* s, double* x, double* u, double* pi, double* lam) {
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    const size_t B = s->B, N = s->N;
    if (x) HIPCHK(hipMemcpy(x, s->x, B * (N + 1) * 12 * sizeof(double), hipMemcpyDeviceToHost));
    if (u) HIPCHK(hipMemcpy(u, s->u, B * N * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (pi) HIPCHK(hipMemcpy(pi, s->pi, B * N * 12 * sizeof(double), hipMemcpyDeviceToHost));
    if (lam) HIPCHK(hipMemcpy(lam, s->lam, B * N * 8 * sizeof(double), hipMemcpyDeviceToHost));
    return BROV_OK;
}
extern "C" int brov_reset(brov_solver* s) {  // acados_solver_bluerov2.c:797-830: everything to zero
    invalidate_preparation(s);
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    const size_t B = s->B, N = s->N;
    HIPCHK(hipMemset(s->x, 0, B * (N + 1) * 12 * sizeof(double)));
    HIPCHK(hipMemset(s->u, 0, B * N * 4 * sizeof(double)));
    HIPCHK(hipMemset(s->pi, 0, B * N * 12 * sizeof(double)));
    HIPCHK(hipMemset(s->lam, 0, B * N * 8 * sizeof(double)));
    // the records too: their u0 / thrust is what a failed step holds, and a reset must not hand the previous run's input on
    HIPCHK(hipMemset(s->res, 0, B * sizeof(brov_result)));
    return BROV_OK;
}

// one RTI step (or half of one) on `st`; `in`: what brov_tick_host has its launch read and write in place of the solver's arrays (null: nothing)
static int solve_phase(brov_solver* s, hipStream_t st, int rti_phase, const LaunchInputs* in) {
    HIPCHK(hipSetDevice(s->device));
    if (int rc = order_behind_last(s, st, in && in->reads_pinned)) return rc;   // e.g. a brov_tick_host whose kernel is still finishing on the solver's own stream
    const SolvePlan plan = plan_solve(s, rti_phase);
    if (rti_phase == 2 && s->prep_path == 0) {   // no preparation, or one that a later step (rti_phase 0, an earlier feedback) has used up: the iterate it linearised is gone
        g_err = "brov_solve: rti_phase 2 needs a preparation (rti_phase 1) of the CURRENT iterate: none since the last step";
        return BROV_ERR_ARG;
    }
    if (rti_phase == 2 && (s->prep_path == 3 || (s->prep_path == 2 && !plan.split_ok))) {   // (a grid / option / iterate / path change between the two calls)
        g_err = "brov_solve: rti_phase 2 after a preparation on the resident kernel, which the solver's settings no longer allow: repeat rti_phase 1";
        return BROV_ERR_ARG;
    }
    if (rti_phase == 1) s->prep_path = plan.prep_path;
    LaunchInputs pred;   // (delay stage: the step and the feedback start from the predicted state; a preparation from the controller's, as ever)
    if (rti_phase != 1) in = predicted_inputs(s, in, pred, st);
    const DevParams P = make_params(s, plan, in);
    time_mark(s, 0, st);
    if (plan.family != FAM_STREAMING) {
        time_mark(s, 1, st);
        launch_lds(s, P, plan.family, st);
    } else {
        if (rti_phase != 2) launch_linearise(P, st);
        time_mark(s, 1, st);
        if (rti_phase != 1) launch_qp(P, st);
        s->pit_ran = false; s->last_family = FAM_STREAMING; s->last_stream = st;
    }
    time_mark(s, 2, st);
    if (rti_phase != 1) s->sched_tick++;   // a QP kernel ran: it wrote the next ordering
    if (rti_phase != 1) s->prep_path = 0;  // ... and the iterate moved (and the per-block workspace was rewritten): whatever preparation there was is used up
    HIPCHK(hipGetLastError());
    return BROV_OK;
}
extern "C" int brov_solve_phase(brov_solver* s, void* stream, int rti_phase) {
    if (!s || rti_phase < 0 || rti_phase > 2) return BROV_ERR_ARG;
    return solve_phase(s, (hipStream_t)stream, rti_phase, nullptr);
}
extern "C" int brov_solve(brov_solver* s, void* stream) { return brov_solve_phase(s, stream, 0); }

// steps in one launch, by family: FAM_FUSED = rti_fused_kernel_ticks (N <= 23), FAM_WINDOWED = rti_window_kernel_ticks (longer horizons, large batches: the windowed kernel's
// persistent blocks), 0 = neither (general grid, streaming pair, a dumped linearisation, the resident / parallel-in-time configurations of small
// batches -- those are latency paths: a launch per step)
static int ticks_kernel(const brov_solver* s) {
    if (s->opts.kernel_path == BROV_PATH_STREAMING || general_grid(s) || s->dump_lin) return 0;
    return serves_fused(s) ? FAM_FUSED : serves_windowed_ticks(s) ? FAM_WINDOWED : 0;
}

// `ticks` RTI steps of every instance with ONE launch where the fused kernels serve the solver (N <= 23, uniform grid): rti_fused_kernel_ticks,
// every instance going on to its next step as soon as its own is done.  Elsewhere (and when the moving window would leave the resident
// table): the same steps as `ticks` launches.  Either way the result equals `ticks` x { brov_set_yref_from_traj(line + k row_stride); brov_solve }.
extern "C" int brov_solve_ticks(brov_solver* s, void* stream, int ticks, int row_stride, int32_t* status_log) {
    if (!s || ticks < 1 || row_stride < 0) { g_err = "brov_solve_ticks: bad argument"; return BROV_ERR_ARG; }
    if (row_stride > 0 && !(s->yref_shared && s->traj && s->traj_line >= 0)) {
        g_err = "brov_solve_ticks: a moving window (row_stride > 0) needs the window in force to come from brov_set_yref_from_traj";
        return BROV_ERR_ARG;
    }
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const int line0 = s->traj_line, ncols = s->traj_ncols;
    const int which = ticks_kernel(s);
    const bool one_launch = which != 0 && (row_stride == 0 || (s->yref_view != nullptr && line0 + (ticks - 1) * row_stride + s->N <= s->traj_rows - 1));
    if (!one_launch) {
        for (int k = 0; k < ticks; k++) {
            if (k > 0 && row_stride > 0)
                if (int rc = brov_set_yref_from_traj(s, line0 + k * row_stride, ncols, stream)) return rc;
            if (int rc = brov_solve_phase(s, stream, 0)) return rc;
            gather_status(s, status_log ? status_log + (size_t)k * s->B : nullptr, st);
        }
        HIPCHK(hipGetLastError());
        return BROV_OK;
    }
    if (int rc = launch_ticks(s, which, ticks, (int64_t)row_stride * 16, status_log, nullptr, st)) return rc;
    HIPCHK(hipGetLastError());
    return BROV_OK;
}

// One control tick with the fewest host round trips (what the acados-shaped drop-in calls per bluerov2_acados_solve): the inputs that
// changed go through ONE pinned staging buffer and asynchronous copies on the solver's own stream, the step is enqueued behind them,
// the result records come back the same way, and the host waits once.  The separate setters + brov_solve + brov_get_results_host
// cost five blocking pageable copies and three synchronisations per tick -- 0.2 .. 0.4 ms at batch 1, more than the kernels.
// the pinned staging buffer of brov_tick_host (TickLayout), (re)allocated on demand
static int tick_pin(brov_solver* s) {
    TickChannel& ch = s->tick;
    const size_t n_all = TickLayout(s->B, s->N).total();
    if (ch.pin_doubles < n_all) {
        if (ch.pin) hipHostFree(ch.pin);
        ch.pin = nullptr; ch.pin_doubles = 0;
        HIPCHK(hipHostMalloc((void**)&ch.pin, n_all * sizeof(double), hipHostMallocDefault));
        ch.pin_doubles = n_all;
        std::memset(ch.pin, 0, ch.pin_doubles * sizeof(double));
    }
    return BROV_OK;
}
// A caller that builds its inputs and reads its records IN these buffers (device-visible pinned host memory, valid until brov_destroy)
// saves brov_tick_host the host-side copies: pass the pointers returned here as x0 / yref_shared / par_stage and NULL as res.
extern "C" int brov_tick_buffers(brov_solver* s, double** x0, double** yref_shared, double** par_stage, const brov_result** res) {
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = tick_pin(s)) return rc;
    TickChannel& ch = s->tick;
    const TickLayout L(s->B, s->N);
    // input set 0 is the caller's from here on and "may be rewritten freely" (header): refresh copies an EARLIER copying tick left running out
    // of set 0 (copy_stream; they read it) must be over before the pointers go out -- the wait at the top of the next brov_tick_host comes
    // after the caller's writes (round-5 advisor)
    if (ch.set_pending[0]) { HIPCHK(hipEventSynchronize(ch.ev_set[0])); ch.set_pending[0] = false; }
    ch.buffers_out = true;
    if (x0) *x0 = ch.pin + L.x0(0);
    if (yref_shared) *yref_shared = ch.pin + L.window(0);
    if (par_stage) *par_stage = ch.pin + L.params(0);
    if (res) *res = (const brov_result*)(ch.pin + L.records());
    return BROV_OK;
}

// How one tick moves its inputs and records: decided here, once per tick, from the call's arguments and the channel's state (no HIP call, no
// side effect).  `passed`: 1 x0, 2 shared window, 4 stage parameters came with the tick.
struct TickPlan {
    int set = 0;                 // input set of the staging buffer the tick uses
    bool mailbox = false, bulk = false;   // records: written by the kernel into the pinned buffer, with / without sequence words
    bool zerocopy = false, behind_copies = false, copies_beside = false;   // inputs: read by the kernel in the pinned buffer; refresh copies
};
static TickPlan plan_tick(int B, int rti_phase, int passed, bool in_place, const DevKnobs& k, bool buffers_out, bool copies_pending, int copy_mask,
                          int pin_sel) {
    TickPlan t;
    // (a caller that holds set 0 through brov_tick_buffers keeps it to itself: its copying ticks, if any, all use set 1)
    t.set = in_place ? 0 : (buffers_out ? 1 : pin_sel ^ 1);
    // Results.  Small batches (the ROS node's batch of one): the kernel writes every record into the pinned buffer itself and then the
    // instance's sequence word; the host polls those words -- no copy command, no stream synchronisation on the way back.  The stream
    // is queried now and then: a launch that ended without delivering (a device fault) falls back to the synchronous path's error.
    // Larger batches: the kernel still writes the records into the pinned buffer itself (no copy command behind it), without the
    // per-instance sequence words -- the host waits for the stream once.
    t.mailbox = rti_phase != 1 && B <= kTickMailboxMaxBatch && k.tick_mailbox;
    t.bulk = !t.mailbox && rti_phase != 1 && B > kTickMailboxMaxBatch && k.tick_mailbox && k.tick_bulk;
    // Inputs.  Small batches with the mailbox: the kernel reads the inputs of this tick where the host has just put them (pinned, device-visible
    // memory: 21 KB over PCIe inside the linearisation's staging loads) instead of waiting for a copy command ahead of it; the device
    // copies every other entry point works on are refreshed by the same copies, enqueued BEHIND the launch (BROV_TICK_ZEROCOPY=0: ahead).
    // Larger batches whose records the kernel writes into the pinned buffer itself (bulk): the same for x0 and a shared window (96 bytes
    // per instance over PCIe inside the linearisation's staging loads) -- not for per-stage parameters passed with the tick (2.7 KB per instance
    // at N = 20: those go through the copy engine ahead of the launch, and the other inputs with them).
    // (a feedback call, rti_phase 2, too: its kernel reads the new measurement where the host has just put it; a preparation never)
    t.zerocopy = (t.mailbox || (t.bulk && !(passed & 4))) && rti_phase != 1 && k.tick_zerocopy;
    // (inputs NOT passed with this tick are read from their device arrays: if the copies an earlier tick left running write one of those, the
    // kernel is ordered behind them after all -- a loop that passes the same inputs every tick never is)
    t.behind_copies = copies_pending && (copy_mask & ~passed) != 0;
    // Large batches (records written by the kernel, the host waits for the launch once): the refresh copies of the tick's inputs run NEXT TO the
    // kernel -- it reads the pinned copies, they write the device arrays, which nothing of this launch reads -- ordered only behind what was
    // enqueued ahead of it.  They are over long before the kernel is (0.4 MB against 0.16 ms), so a caller that owns the staging buffers
    // (brov_tick_buffers) does not pay for them at the end of the call.  Small batches keep them BEHIND the kernel: next to it they would share
    // the PCIe reads of a 50 us launch whose latency is the point.
    t.copies_beside = t.zerocopy && t.bulk && !t.behind_copies;
    return t;
}
// The inputs passed with the tick into input set `set` of the staging buffer, and what the solver remembers of them.
// The refresh copies a zero-copy tick leaves running behind its kernel (pinned staging buffer -> device arrays, copy_stream) still READ the
// input set they were enqueued for (round-4 advisor: rewriting it under them leaves a torn or already-next-tick x0 in the device array).
// Waiting for them at the top of the next tick costs a back-to-back control loop 30 us (the kernel's tail and the copies behind it; measured,
// round 5) -- so the staging buffer holds TWO input sets and ticks that copy their arguments in alternate: a set is rewritten two ticks
// after its copies were enqueued, and the check below almost always finds them done.
static int stage_inputs(brov_solver* s, const TickLayout& L, int set, const double* x0, const double* yref_shared, const double* par_stage) {
    TickChannel& ch = s->tick;
    if (ch.set_pending[set] && hipEventQuery(ch.ev_set[set]) != hipSuccess) {
        (void)hipGetLastError();
        HIPCHK(hipEventSynchronize(ch.ev_set[set]));
    }
    ch.set_pending[set] = false;
    double *px = ch.pin + L.x0(set), *py = ch.pin + L.window(set), *pp = ch.pin + L.params(set);
    if (x0 && x0 != px) std::memcpy(px, x0, L.n_x0 * sizeof(double));   // (equal: the caller wrote into the staging buffer, brov_tick_buffers)
    if (yref_shared) {
        if (yref_shared != py) std::memcpy(py, yref_shared, L.n_y * sizeof(double));
        forget_traj_window(s);
        s->yref_shared = true;
    }
    if (par_stage) { if (par_stage != pp) std::memcpy(pp, par_stage, L.n_p * sizeof(double)); s->plant.params_changed(); }
    return BROV_OK;
}
// the inputs `passed` with a tick from input set `set` to the device arrays every other entry point works on, on `cs`
static int upload_inputs(brov_solver* s, const TickLayout& L, int set, int passed, hipStream_t cs) {
    const double* pin = s->tick.pin;
    if (passed == 7) {   // device side: one allocation in the same order (brov_create)
        HIPCHK(hipMemcpyAsync(s->x0, pin + L.x0(set), L.inputs() * sizeof(double), hipMemcpyHostToDevice, cs));
    } else {
        if (passed & 1) HIPCHK(hipMemcpyAsync(s->x0, pin + L.x0(set), L.n_x0 * sizeof(double), hipMemcpyHostToDevice, cs));
        if (passed & 2) HIPCHK(hipMemcpyAsync(s->yref_sh, pin + L.window(set), L.n_y * sizeof(double), hipMemcpyHostToDevice, cs));
        if (passed & 4) HIPCHK(hipMemcpyAsync(s->par, pin + L.params(set), L.n_p * sizeof(double), hipMemcpyHostToDevice, cs));
    }
    return BROV_OK;
}
// Ahead of the launch: the uploads of a tick whose kernel reads the device arrays; what a zero-copy tick needs behind it, on first use.
static int enqueue_ahead(brov_solver* s, const TickLayout& L, const TickPlan& t, int passed, int rti_phase) {
    TickChannel& ch = s->tick;
    if (!t.zerocopy) {
        if (ch.copies_pending) HIPCHK(hipStreamWaitEvent(ch.stream, ch.ev_copy, 0));   // (an earlier tick's copies into the same device arrays)
        if (int rc = upload_inputs(s, L, t.set, passed, ch.stream)) return rc;
        if (rti_phase == 1) {   // a preparation delivers nothing: the call returns when the staging buffer is free again (wait_records), not when the kernel ends
            if (!ch.ev_up) HIPCHK(hipEventCreateWithFlags(&ch.ev_up, hipEventDisableTiming));
            HIPCHK(hipEventRecord(ch.ev_up, ch.stream));
        }
    } else if (!ch.copy_stream) {
        HIPCHK(hipStreamCreateWithFlags(&ch.copy_stream, hipStreamNonBlocking));
        for (hipEvent_t* e : {&ch.ev_tick, &ch.ev_pre, &ch.ev_set[0], &ch.ev_set[1]}) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        ch.ev_copy = ch.ev_set[0];
    }
    return BROV_OK;
}
// what the tick's launch reads and writes in the staging buffer
static LaunchInputs tick_launch_inputs(const TickChannel& ch, const TickLayout& L, const TickPlan& t, int passed) {
    LaunchInputs in;
    if (t.zerocopy) {
        if (passed & 1) in.x0 = ch.pin + L.x0(t.set);
        if (passed & 2) in.yref = ch.pin + L.window(t.set);
        if (passed & 4) in.par = ch.pin + L.params(t.set);
    }
    if (t.mailbox || t.bulk) in.mail = (brov_result*)(ch.pin + L.records());
    if (t.mailbox) in.mail_flag = (int32_t*)(ch.pin + L.seq_words());
    in.mail_seq = ch.mail_seq;
    in.reads_pinned = t.zerocopy && !t.behind_copies;
    return in;
}
// Behind the launch of a zero-copy tick: the device copies every other entry point works on are refreshed BEHIND the kernel that has read the
// pinned ones (copies_beside: next to it), on the copy stream -- neither the host (which waits for the kernel's end / the mailbox) nor the next
// tick's kernel waits for them; whatever else touches those arrays is ordered behind ev_copy (order_behind_last, sync_last)
static int enqueue_behind(brov_solver* s, const TickLayout& L, const TickPlan& t, int passed) {
    TickChannel& ch = s->tick;
    HIPCHK(hipEventRecord(ch.ev_tick, ch.stream));
    HIPCHK(hipStreamWaitEvent(ch.copy_stream, t.copies_beside ? ch.ev_pre : ch.ev_tick, 0));
    if (int rc = upload_inputs(s, L, t.set, passed, ch.copy_stream)) return rc;
    ch.ev_copy = ch.ev_set[t.set];
    HIPCHK(hipEventRecord(ch.ev_copy, ch.copy_stream));
    ch.set_pending[t.set] = true;
    ch.copy_mask = (ch.copies_pending && !t.behind_copies) ? (ch.copy_mask | passed) : passed;   // (arrays written by copies no kernel on the tick's stream is ordered behind yet)
    ch.copies_pending = true;
    return BROV_OK;
}
// The host's one wait: for the records in the pinned buffer (mailbox poll / the kernel's end / the stream with the copy back behind the
// kernel), or, a preparation, for the inputs to have left it -- the preparation itself runs on, stream-ordered ahead of whatever follows
static int wait_records(brov_solver* s, const TickLayout& L, const TickPlan& t, int rti_phase) {
    TickChannel& ch = s->tick;
    const size_t B = s->B;
    if (t.mailbox) {
        const volatile int32_t* pf = (const volatile int32_t*)(ch.pin + L.seq_words());
        const int32_t seq = ch.mail_seq;
        size_t done = 0;
        for (unsigned long spin = 1; done < B; spin++) {
            while (done < B && pf[done] == seq) done++;
            if (done < B && (spin & 0x3ff) == 0) {
                const hipError_t q = hipStreamQuery(ch.stream);
                if (q == hipSuccess) {   // the launch is over: everything it wrote is visible
                    while (done < B && pf[done] == seq) done++;
                    if (done < B) { g_err = "brov_tick_host: the solve ended without delivering its records"; return BROV_ERR_HIP; }
                } else if (q != hipErrorNotReady) {
                    g_err = std::string("brov_tick_host: ") + hipGetErrorString(q);
                    return BROV_ERR_HIP;
                }
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    } else if (rti_phase == 1) {
        HIPCHK(hipEventSynchronize(ch.ev_up));
    } else {
        if (!t.bulk) HIPCHK(hipMemcpyAsync(ch.pin + L.records(), s->res, B * sizeof(brov_result), hipMemcpyDeviceToHost, ch.stream));
        if (t.zerocopy) HIPCHK(hipEventSynchronize(ch.ev_tick));
        else HIPCHK(hipStreamSynchronize(ch.stream));
    }
    return BROV_OK;
}

extern "C" int brov_tick_host(brov_solver* s, const double* x0, const double* yref_shared, const double* par_stage, int rti_phase,
                              brov_result* res) {
    if (!s || rti_phase < 0 || rti_phase > 2) return BROV_ERR_ARG;
    if (x0 && s->plant.dl.predicts()) {
        g_err = "brov_tick_host: the delay stage predicts the solve's initial state from the controller's own (comp > 0, brov_delay_set_host): "
                "a tick that brings its own x0 is refused";
        return BROV_ERR_ARG;
    }
    using clk = std::chrono::steady_clock;
    const bool brk = s->k.tick_breakdown != 0;
    clk::time_point tb0, tb1, tb2, tb3, tb4;
    if (brk) tb0 = clk::now();
    HIPCHK(hipSetDevice(s->device));
    TickChannel& ch = s->tick;
    const TickLayout L(s->B, s->N);
    if (!ch.stream) HIPCHK(hipStreamCreateWithFlags(&ch.stream, hipStreamNonBlocking));
    if (int rc = tick_pin(s)) return rc;
    hipStream_t st = ch.stream;
    if (s->last_stream != st) HIPCHK(sync_last(s));   // an earlier solve on the caller's stream
    const int passed = (x0 ? 1 : 0) | (yref_shared ? 2 : 0) | (par_stage ? 4 : 0);
    const bool in_place = (x0 && x0 == ch.pin + L.x0(0)) || (yref_shared && yref_shared == ch.pin + L.window(0)) || (par_stage && par_stage == ch.pin + L.params(0));
    const TickPlan t = plan_tick(s->B, rti_phase, passed, in_place, s->k, ch.buffers_out, ch.copies_pending, ch.copy_mask, ch.pin_sel);
    if (!in_place && !ch.buffers_out) ch.pin_sel = t.set;   // copying ticks alternate between the two input sets
    if (int rc = stage_inputs(s, L, t.set, x0, yref_shared, par_stage)) return rc;
    if (int rc = enqueue_ahead(s, L, t, passed, rti_phase)) return rc;
    if (t.mailbox) ch.mail_seq = ch.mail_seq == 0x7fffffff ? 1 : ch.mail_seq + 1;
    LaunchInputs in = tick_launch_inputs(ch, L, t, passed);   // a local: no path out of this call leaves a later solve reading the pinned buffer
    in.x0 = s->plant.tick_state(passed & 1, in.x0);   // sensor stage on: an x0 copied in ahead of the launch is the caller's measurement, as one read in place is
    if (brk) tb1 = clk::now();
    if (t.copies_beside) HIPCHK(hipEventRecord(ch.ev_pre, st));   // (ahead of the launch like enqueue_ahead, but on the launch's side of the breakdown)
    const int rc = solve_phase(s, st, rti_phase, &in);
    if (brk) tb2 = clk::now();
    if (rc) return rc;
    if (t.zerocopy) { if (int rc2 = enqueue_behind(s, L, t, passed)) return rc2; }
    if (brk) tb3 = clk::now();
    if (int rc2 = wait_records(s, L, t, rti_phase)) return rc2;
    if (rti_phase == 1) return BROV_OK;   // (no record: `res` is left alone)
    if (brk) {
        tb4 = clk::now();
        auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        ch.tick_us[0] = us(tb0, tb1); ch.tick_us[1] = us(tb1, tb2); ch.tick_us[2] = us(tb2, tb3); ch.tick_us[3] = us(tb3, tb4); ch.tick_us[4] = us(tb0, tb4);
    }
    const brov_result* pr = (const brov_result*)(ch.pin + L.records());
    if (res && res != pr) std::memcpy(res, pr, s->B * sizeof(brov_result));
    // a caller that builds its inputs IN the staging buffers (brov_tick_buffers) is free to write the next tick's as soon as this call is back:
    // the refresh copies out of them are over by then
    if (t.zerocopy && in_place) HIPCHK(hipEventSynchronize(ch.ev_copy));
    return BROV_OK;
}

extern "C" int brov_set_opts(brov_solver* s, const brov_opts* o) {
    invalidate_preparation(s);
    if (!s || !o || o->N != s->N) { g_err = "brov_set_opts: bad argument (N is fixed at create)"; return BROV_ERR_ARG; }
    if (const char* why = opts_problem(o)) { g_err = std::string("brov_set_opts: ") + why; return BROV_ERR_ARG; }
    if (o->kernel_path == BROV_PATH_FUSED && !serves_fused(s) && !s->ws) {
        // the windowed kernel's workspace is allocated at create, from the path and batch asked for then
        g_err = "brov_set_opts: BROV_PATH_FUSED at this horizon needs the windowed kernel's workspace, which this solver was created without "
                "(created with BROV_PATH_STREAMING): create it with BROV_PATH_AUTO or BROV_PATH_FUSED";
        return BROV_ERR_ARG;
    }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    s->opts = *o;
    return upload_cst(s);
}
extern "C" int brov_get_opts(const brov_solver* s, brov_opts* o) {
    if (!s || !o) return BROV_ERR_ARG;
    *o = s->opts;
    return BROV_OK;
}
extern "C" int brov_synchronize(brov_solver* s, void* stream) {
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return BROV_OK;
}
extern "C" int brov_last_kernel_path(const brov_solver* s) {
    return s ? (s->last_family == FAM_FUSED ? BROV_PATH_FUSED : (s->last_family == FAM_WINDOWED ? BROV_PATH_WINDOWED : BROV_PATH_STREAMING)) : BROV_ERR_ARG;
}
// which instances of the LAST solve were completed by the parallel-in-time kernel (rti_pit_kernel, batches the resident windowed mode
// serves): done[b] = 1, else 0 -- all zero when that kernel did not run.  Test / bench instrumentation.
// development (BROV_TICK_BREAKDOWN=1 at create): host time of the last brov_tick_host in microseconds -- [0] entry to launch (device selection,
// staging: copies into the pinned buffer, waits for earlier refresh copies), [1] solve_phase (parameter block, kernel launch(es)), [2] what is
// enqueued behind the launch (events, refresh copies), [3] the wait for the records (mailbox poll / event / stream), [4] the whole call
extern "C" int brov_dev_tick_breakdown(brov_solver* s, double us[5]) {
    if (!s || !us) return BROV_ERR_ARG;
    for (int k = 0; k < 5; k++) us[k] = s->tick.tick_us[k];
    return BROV_OK;
}
extern "C" int brov_pit_last(brov_solver* s, int32_t* done) {
    if (!s || !done) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    if (!s->pit_ran) { std::memset(done, 0, (size_t)s->B * sizeof(int32_t)); return BROV_OK; }
    HIPCHK(hipMemcpy(done, s->pit_done, (size_t)s->B * sizeof(int32_t), hipMemcpyDeviceToHost));
    return BROV_OK;
}
extern "C" int brov_lds_kernel_info(const brov_solver* s, int32_t info[4]) {
    if (!s || !info) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    const bool fused = serves_fused(s);
    // streaming kernels (asked for, or forced by a general grid, or no windowed workspace): stage blocks in HBM, nothing to report
    if (s->opts.kernel_path == BROV_PATH_STREAMING || (!fused && !s->ws)) { info[0] = info[1] = info[2] = info[3] = 0; return BROV_OK; }
    lds_kernel_info(s->N, s->win_L, !fused, info, s->k);
    return BROV_OK;
}
extern "C" int brov_window_stages(const brov_solver* s) { return s ? (s->ws ? s->win_L : 0) : BROV_ERR_ARG; }
extern "C" int brov_debug_dump_linearisation(brov_solver* s, int enable) {
    if (!s) return BROV_ERR_ARG;
    s->dump_lin = enable != 0;
    return BROV_OK;
}
// developer hook (not in the public header): per-instance phase timestamps of the last solve, 8 x uint64 per instance
extern "C" int brov_debug_phase_stamps(brov_solver* s, int enable, unsigned long long* out_host) {
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    // [B][8] phase stamps followed by [B][8] interior-point phase totals (the latter only filled by a -DBROV_DBG_IPM build)
    if (enable && !s->dbg) { HIPCHK(hipMalloc((void**)&s->dbg, (size_t)s->B * 128)); HIPCHK(hipMemset(s->dbg, 0, (size_t)s->B * 128)); }
    if (out_host && s->dbg) HIPCHK(hipMemcpy(out_host, s->dbg, (size_t)s->B * (enable == 2 ? 128 : 64), hipMemcpyDeviceToHost));
    if (!enable && s->dbg) { hipFree(s->dbg); s->dbg = nullptr; }
    return BROV_OK;
}
extern "C" int brov_enable_timing(brov_solver* s, int on) { if (!s) return BROV_ERR_ARG; s->timing = on != 0; s->ev_valid = false; return BROV_OK; }
extern "C" int brov_last_solve_seconds(brov_solver* s, double* total, double* k2) {
    if (!s || !s->ev_valid) return BROV_ERR_ARG;
    HIPCHK(hipEventSynchronize(s->ev[2]));
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
    HIPCHK(hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
    if (total) *total = (a + b) * 1e-3;
    if (k2) { k2[0] = a * 1e-3; k2[1] = b * 1e-3; }
    return BROV_OK;
}

extern "C" int brov_get_results_host(brov_solver* s, brov_result* res) {
    if (!s || !res) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    HIPCHK(hipMemcpy(res, s->res, (size_t)s->B * sizeof(brov_result), hipMemcpyDeviceToHost));
    return BROV_OK;
}
extern "C" int brov_get_u0_host(brov_solver* s, double* u0) {
    if (!s || !u0) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    HIPCHK(hipMemcpy2D(u0, 4 * sizeof(double), s->res, sizeof(brov_result), 4 * sizeof(double), s->B, hipMemcpyDeviceToHost));
    return BROV_OK;
}
extern "C" const brov_result* brov_results_device(const brov_solver* s) { return s ? s->res : nullptr; }
extern "C" double* brov_x0_device(brov_solver* s) { return s ? s->x0 : nullptr; }
namespace brov {
// what the controller knows of the state: the measured state while the sensor stage is on, else the plant's own (for the observer and the estimator)
const double* solver_measured_state(const brov_solver* s) { return s ? s->plant.controller_state() : nullptr; }
// the records whose thrusts the observer is fed: the commanded ones, unless the thrust-curve stage (the last to rewrite the record), the
// rotor stage or the delay stage is on with observer_applied set
const brov_result* solver_observer_results(const brov_solver* s) {
    if (!s) return nullptr;
    if (s->plant.cv.on && s->plant.cv.observer_applied) return s->plant.cv.applied;   // behind the rotors, or in their place
    if (s->plant.ro.on && s->plant.ro.observer_applied) return s->plant.ro.applied;
    return s->plant.dl.on && s->plant.dl.observer_applied ? s->plant.dl.applied : s->res;
}
ImuView solver_imu_view(const brov_solver* s) {
    ImuView v;
    if (!s || !s->plant.im.on) return v;
    const ImuSource& im = s->plant.im;
    v.on = true; v.fix_due = im.fix_due; v.h = im.par.h;
    v.imu = im.out.imu; v.gps_p = im.out.gps_p; v.gps_v = im.out.gps_v; v.qm = im.out.qm; v.fix = im.out.fix;
    return v;
}
void launch_copy_stage0_par(const double* par, double* pp, int B, int N1, hipStream_t st) {   // for SolverPlant::ensure_params
    hipLaunchKernelGGL(copy_stage0_par_kernel, dim3((B * 16 + 255) / 256), dim3(256), 0, st, par, pp, B, N1);
}
}  // namespace brov
extern "C" double* brov_yref_device(brov_solver* s) { if (!s) return nullptr; s->yref_shared = false; forget_traj_window(s); return s->yref; }
extern "C" double* brov_params_device(brov_solver* s) { if (!s) return nullptr; s->plant.params_changed(); return s->par; }
extern "C" double* brov_x_device(brov_solver* s) { return s ? s->x : nullptr; }
extern "C" double* brov_u_device(brov_solver* s) { return s ? s->u : nullptr; }

extern "C" int brov_get_linearisation_host(brov_solver* s, double* AB, double* b) {
    if (!s) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    if (AB) HIPCHK(hipMemcpy(AB, s->BA, (size_t)s->B * s->N * 192 * sizeof(double), hipMemcpyDeviceToHost));
    if (b) HIPCHK(hipMemcpy(b, s->bvec, (size_t)s->B * s->N * 12 * sizeof(double), hipMemcpyDeviceToHost));
    return BROV_OK;
}

// arg-min of cost over the eligible instances (select_device.hpp: status SUCCESS and a finite cost): one block, strided scan + block_argmin
__global__ __launch_bounds__(256) void select_best_kernel(const brov_result* __restrict__ res, int B, int* __restrict__ out) {
    double best = 0.0;
    int bi = -1;
    for (int k = threadIdx.x; k < B; k += blockDim.x)   // ascending: within a thread an equal cost never replaces an earlier index
        if (result_eligible(res[k].status, res[k].cost)) argmin_next(best, bi, res[k].cost, k);
    block_argmin<256>(best, bi);
    if (threadIdx.x == 0) out[0] = bi;
}

extern "C" int brov_select_best_host(brov_solver* s, int* best_index, brov_result* best) {
    if (!s || !best_index) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    hipLaunchKernelGGL(select_best_kernel, dim3(1), dim3(256), 0, s->last_stream, s->res, s->B, s->best);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_last(s));
    int idx = -1;
    HIPCHK(hipMemcpy(&idx, s->best, sizeof(int), hipMemcpyDeviceToHost));
    *best_index = idx;
    if (best && idx >= 0) HIPCHK(hipMemcpy(best, s->res + idx, sizeof(brov_result), hipMemcpyDeviceToHost));
    return BROV_OK;
}

extern "C" int brov_get_thrusts_host(brov_solver* s, double* t6) {
    if (!s || !t6) return BROV_ERR_ARG;
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(sync_last(s));
    HIPCHK(hipMemcpy2D(t6, 6 * sizeof(double), (const char*)s->res + offsetof(brov_result, thrust), sizeof(brov_result), 6 * sizeof(double),
                       s->B, hipMemcpyDeviceToHost));
    return BROV_OK;
}
