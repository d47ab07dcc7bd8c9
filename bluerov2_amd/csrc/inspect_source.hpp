// inspect_source.hpp -- the host side of the range stage and the inspection controller (inspect_kernel.hip: range_eval_kernel,
// inspect_eval_kernel, inspect_tick_kernel; the public names are brov_range_* and brov_inspect_* of include/bluerov2_nmpc_inspect.h): the scene
// and the camera in force -- both travel in the kernel arguments --, the per-instance noise, the controller's parameters, its state and
// statistics on the device, the last range and status, and the timing of the last launches.  Its owner is a brov_solver, whose entry points
// check their own handle and forward here with the owner's call context (CallCtx, host_common.hpp) as they do for the IMU stage, whose shape
// this follows.  `on` is the controller: while it is on, brov_inspect_step writes the solver's records.  Host code only, header only.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "nmpc_device.hpp"
#include "mesh_source.hpp"

namespace brov {

struct InspectSource : PlantStage {
    static constexpr long long kMaxIndex = 1LL << 24;   // the measurement index has 24 bits of the noise counter
    brov_range_params cam = default_range();
    RangeScene scene{};
    MeshSource mesh;                    // the triangle mesh beside the boxes (brov_mesh_*): while one is set the mesh kernels cast the rays
    brov_inspect_params ctl = default_inspect();
    InspectDev dev;
    double* sigma = nullptr;            // [B]
    double* eval_d = nullptr;           // [B][12 + 1 + 9 + 3] of the eval calls: x, range, rot | range, z, psi
    int32_t* eval_hits = nullptr;       // [B]
    brov_inspect_state* eval_state = nullptr;   // [2][B]
    brov_inspect_stats* eval_stats = nullptr;   // [B]
    brov_result* eval_rec = nullptr;    // [B]
    KernelTimer rtimer;                 // around the last launch that cast rays (timer: around the tick kernel's)

    static brov_range_params default_range() {
        brov_range_params p{};
        p.f = focal(1280.0, 85.2 * M_PI / 180.0);
        p.near = 0.1; p.far = 100.0; p.roi = 40;
        return p;
    }
    static double focal(double width, double hfov) { return width / (2.0 * std::tan(hfov / 2.0)); }
    static brov_inspect_params default_inspect() {
        brov_inspect_params p{};
        p.dt = 0.05; p.safety_dis = 1.79; p.buffer = 0.5; p.sway = -4.0; p.sway_slow = -2.0; p.surge_search = 1.0; p.z0 = -34.5;
        p.yaw0 = 0.5 * M_PI;
        p.dz_round = p.safety_dis * std::tan(32 * M_PI / 180) * 2;
        p.lost = 0.1; p.yaw_tol = 0.1; p.yaw_home_tol = 0.2; p.z_tol = 0.25; p.height_tol = 0.1; p.t_hold = 1.0;
        p.z_goal = p.z0 + p.dz_round;
        const double g[9] = {5, 0, 0, 5, 0, 0, 7, 0.08, 0};
        for (int i = 0; i < 9; i++) p.gains[i] = g[i];
        p.flags = BROV_INSPECT_SHARED_PID | BROV_INSPECT_FLOAT_YAW;
        return p;
    }
    // the state of the node's constructor
    brov_inspect_state initial_state() const {
        brov_inspect_state s{};
        const double y = (ctl.flags & BROV_INSPECT_FLOAT_YAW) ? (double)(float)ctl.yaw0 : ctl.yaw0;
        s.yaw_sum = y; s.pre_yaw = y; s.ref_x = ctl.safety_dis; s.ref_z = ctl.z0; s.ref_yaw = ctl.yaw0;
        s.completed_turn = 1; s.get_height = 1;
        return s;
    }
    static brov_inspect_stats initial_stats() {
        brov_inspect_stats t{};
        t.first_done = -1;
        return t;
    }

    void destroy() { mesh.destroy(); rtimer.destroy(); PlantStage::destroy(); }
    static int index_ok(long long m, const CallCtx& c) {
        if (m < 0 || m >= kMaxIndex) return c.refuse("the range stage's measurement index (the plant's tick counter) must stay in [0, 2^24)");
        return BROV_OK;
    }
    // with the controller on: a plant step of length `dt`?  The controller's time, integral and derivative are in steps of its own dt
    int dt_ok(double dt, const CallCtx& c) const {
        return on && dt != ctl.dt ? c.refuse("the inspection controller is on and dt is not its period (brov_inspect_set_host)") : BROV_OK;
    }
    // may `n` ticks of the loop run from the counter's value `tick`, behind a delay stage that predicts `comp` steps?
    int steps_ok(long long tick, long long n, int comp, const CallCtx& c) const {
        if (!on) return c.refuse("the inspection controller is off (brov_inspect_set_host)");
        if (scene.n < 1 && !mesh.set()) return c.refuse("the scene has no box (brov_range_set_scene_host)");
        if (comp > 0) return c.refuse("the delay stage predicts comp > 0 steps ahead (brov_delay_set_host): the controller has no solve to predict for");
        return index_ok(tick + n - 1, c);
    }

    int ensure(const CallCtx& c) {
        if (int rc = buffer(&sigma, B, c)) return rc;
        if (!rtimer.ev[0]) BROV_HIPCHK(c.err, rtimer.create());
        if (int rc = buffer(&dev.range, B, c)) return rc;
        if (int rc = buffer(&dev.status, B, c)) return rc;
        if (int rc = buffer(&eval_d, B * 25, c)) return rc;
        if (int rc = buffer(&eval_hits, B, c)) return rc;
        if (int rc = buffer(&eval_state, 2 * B, c)) return rc;
        if (int rc = buffer(&eval_stats, B, c)) return rc;
        if (int rc = buffer(&eval_rec, B, c)) return rc;
        const bool fresh = !dev.state;
        if (int rc = buffer(&dev.state, B, c)) return rc;
        if (int rc = buffer(&dev.stats, B, c)) return rc;
        if (fresh) {
            if (int rc = upload_state(c.err)) return rc;
            if (int rc = upload_stats(c.err)) return rc;
        }
        configured = true;
        return BROV_OK;
    }
    int ready(const CallCtx& c) { const int rc = c.wait(); return rc ? rc : ensure(c); }
    int upload_state(std::string& err) {
        const std::vector<brov_inspect_state> s0(B, initial_state());
        BROV_HIPCHK(err, hipMemcpy(dev.state, s0.data(), B * sizeof(brov_inspect_state), hipMemcpyHostToDevice));
        BROV_HIPCHK(err, hipMemset(dev.range, 0, B * sizeof(double)));
        BROV_HIPCHK(err, hipMemset(dev.status, 0, B * sizeof(int32_t)));
        return BROV_OK;
    }
    int upload_stats(std::string& err) {
        const std::vector<brov_inspect_stats> t0(B, initial_stats());
        BROV_HIPCHK(err, hipMemcpy(dev.stats, t0.data(), B * sizeof(brov_inspect_stats), hipMemcpyHostToDevice));
        return BROV_OK;
    }

    // ---- the range stage ------------------------------------------------------------------------------------------------------------
    int set_scene_host(int32_t n, const double* lo, const double* hi, const CallCtx& c) {
        if (n < 0 || n > BROV_RANGE_MAX_BOXES) return c.refuse("the scene holds 0 ... BROV_RANGE_MAX_BOXES boxes");
        if (n > 0 && (!lo || !hi)) return c.refuse("null argument");
        for (int j = 0; j < n * 3; j++) {
            if (!std::isfinite(lo[j]) || !std::isfinite(hi[j])) return c.refuse("a box bound is not finite");
            if (lo[j] > hi[j]) return c.refuse("lo > hi: a box is empty");
        }
        if (int rc = c.wait()) return rc;
        RangeScene sc{};
        for (int k = 0; k < n; k++)
            for (int a = 0; a < 3; a++) { sc.lo[k][a] = lo[k * 3 + a]; sc.hi[k][a] = hi[k * 3 + a]; }
        sc.n = n;
        scene = sc;
        return BROV_OK;
    }
    int set_range_host(const brov_range_params* p, const double* sigma_h, const CallCtx& c) {
        if (!p) return c.refuse("null argument");
        if (p->roi < 2 || p->roi > 64 || (p->roi & 1)) return c.refuse("roi must be even and lie in 2 ... 64");
        const double v[8] = {p->f, p->cx, p->cy, p->mount[0], p->mount[1], p->mount[2], p->near, p->far};
        for (double q : v)
            if (!std::isfinite(q)) return c.refuse("a camera parameter is not finite");
        if (!(p->f > 0.0)) return c.refuse("f must be positive");
        if (!(p->near < p->far)) return c.refuse("near must be below far");
        for (size_t b = 0; sigma_h && b < B; b++)
            if (!(sigma_h[b] >= 0.0)) return c.refuse("sigma must be >= 0 (and not NaN)");
        if (int rc = ready(c)) return rc;
        if (sigma_h) BROV_HIPCHK(c.err, hipMemcpy(sigma, sigma_h, B * sizeof(double), hipMemcpyHostToDevice));
        else BROV_HIPCHK(c.err, hipMemset(sigma, 0, B * sizeof(double)));
        cam = *p;
        cam.reserved_ = 0;
        return BROV_OK;
    }
    // visits: [B][2] node tests and triangle tests per instance (brov_mesh_eval_host, which needs a mesh: need_mesh), or nullptr
    int range_eval_host(int64_t m, const double* x, double* range, int32_t* hits, double* rot, double* depth, const hipStream_t& st, const CallCtx& c,
                        int64_t* visits = nullptr, bool need_mesh = false) {
        if (!x || !range || !hits) return c.refuse("null argument");
        if (need_mesh && !mesh.set()) return c.refuse("no mesh is set (brov_mesh_set_host)");
        if (int rc = index_ok((long long)m, c)) return rc;
        if (int rc = ready(c)) return rc;
        double *xd = eval_d, *rd = eval_d + B * 12, *rotd = eval_d + B * 13;
        const size_t rays = (size_t)cam.roi * cam.roi;
        ScopedDeviceBuffer<double> dd;
        if (depth) BROV_HIPCHK(c.err, dd.init(B * rays));
        ScopedDeviceBuffer<long long> vd;
        if (visits) BROV_HIPCHK(c.err, vd.init(B * 2));
        BROV_HIPCHK(c.err, hipMemcpy(xd, x, B * 12 * sizeof(double), hipMemcpyHostToDevice));
        (void)rtimer.start(st);
        if (mesh.set()) launch_mesh_eval(cam, scene, mesh.dev, sigma, (int)B, (long long)m, xd, rd, eval_hits, rot ? rotd : nullptr, dd.p, vd.p, st);
        else launch_range_eval(cam, scene, sigma, (int)B, (long long)m, xd, rd, eval_hits, rot ? rotd : nullptr, dd.p, st);
        (void)rtimer.stop(st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        BROV_HIPCHK(c.err, hipMemcpy(range, rd, B * sizeof(double), hipMemcpyDeviceToHost));
        BROV_HIPCHK(c.err, hipMemcpy(hits, eval_hits, B * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (rot) BROV_HIPCHK(c.err, hipMemcpy(rot, rotd, B * 9 * sizeof(double), hipMemcpyDeviceToHost));
        if (depth) BROV_HIPCHK(c.err, hipMemcpy(depth, dd.p, B * rays * sizeof(double), hipMemcpyDeviceToHost));
        if (visits) BROV_HIPCHK(c.err, hipMemcpy(visits, vd.p, B * 2 * sizeof(long long), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int range_last_seconds(double* seconds, const CallCtx& c) {
        if (!seconds || !rtimer.valid) return c.refuse(seconds ? "no launch of the range stage yet" : "null argument");
        return rtimer.seconds(seconds, c.err);
    }

    // ---- the controller -----------------------------------------------------------------------------------------------------------------
    int set_host(const brov_inspect_params* p, const CallCtx& c) {
        if (!p) return c.refuse("null argument");
        const double* v = &p->dt;   // the 16 scalars and the 9 gains are 25 doubles in a row
        for (int j = 0; j < 25; j++)
            if (!std::isfinite(v[j])) return c.refuse("a parameter is not finite");
        if (!(p->dt > 0.0)) return c.refuse("dt must be positive");
        if (p->flags & ~(BROV_INSPECT_SHARED_PID | BROV_INSPECT_FLOAT_YAW)) return c.refuse("unknown flag");
        if (int rc = ready(c)) return rc;
        ctl = *p;
        ctl.reserved_ = 0;
        if (int rc = upload_state(c.err)) return rc;
        if (int rc = upload_stats(c.err)) return rc;
        on = true;
        return BROV_OK;
    }
    int reset(const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        return upload_state(c.err);
    }
    int reset_stats(const CallCtx& c) {
        if (int rc = ready(c)) return rc;
        return upload_stats(c.err);
    }
    int eval_host(const brov_inspect_state* state_in, const double* range, const double* z, const double* psi, brov_inspect_state* state_out,
                  brov_result* rec, brov_inspect_stats* stats, const hipStream_t& st, const CallCtx& c) {
        if (!state_in || !range || !z || !psi || !state_out || !rec) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        double *rd = eval_d + B * 22, *zd = rd + B, *pd = zd + B;
        BROV_HIPCHK(c.err, hipMemcpy(eval_state, state_in, B * sizeof(brov_inspect_state), hipMemcpyHostToDevice));
        BROV_HIPCHK(c.err, hipMemcpy(rd, range, B * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(c.err, hipMemcpy(zd, z, B * sizeof(double), hipMemcpyHostToDevice));
        BROV_HIPCHK(c.err, hipMemcpy(pd, psi, B * sizeof(double), hipMemcpyHostToDevice));
        if (stats) BROV_HIPCHK(c.err, hipMemcpy(eval_stats, stats, B * sizeof(brov_inspect_stats), hipMemcpyHostToDevice));
        launch_inspect_eval(ctl, (int)B, eval_state, rd, zd, pd, eval_state + B, eval_rec, stats ? eval_stats : nullptr, st);
        BROV_HIPCHK(c.err, hipGetLastError());
        BROV_HIPCHK(c.err, hipStreamSynchronize(st));
        BROV_HIPCHK(c.err, hipMemcpy(state_out, eval_state + B, B * sizeof(brov_inspect_state), hipMemcpyDeviceToHost));
        BROV_HIPCHK(c.err, hipMemcpy(rec, eval_rec, B * sizeof(brov_result), hipMemcpyDeviceToHost));
        if (stats) BROV_HIPCHK(c.err, hipMemcpy(stats, eval_stats, B * sizeof(brov_inspect_stats), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_state_host(brov_inspect_state* state, double* range, const CallCtx& c) {
        if (!state && !range) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        if (state) BROV_HIPCHK(c.err, hipMemcpy(state, dev.state, B * sizeof(brov_inspect_state), hipMemcpyDeviceToHost));
        if (range) BROV_HIPCHK(c.err, hipMemcpy(range, dev.range, B * sizeof(double), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int get_stats_host(brov_inspect_stats* stats, const CallCtx& c) {
        if (!stats) return c.refuse("null argument");
        if (int rc = ready(c)) return rc;
        BROV_HIPCHK(c.err, hipMemcpy(stats, dev.stats, B * sizeof(brov_inspect_stats), hipMemcpyDeviceToHost));
        return BROV_OK;
    }
    int last_seconds(double* seconds, const CallCtx& c) { return PlantStage::last_seconds(seconds, "no tick of the inspection controller yet", c); }

    // one tick at index `m` on `st` (the owner has asked steps_ok): rays from the true state `x`, the controller on z and psi of `y`, the
    // record into `res`; timed
    void step(const double* x, const double* y, brov_result* res, long long m, hipStream_t st) {
        (void)timer.start(st);
        (void)rtimer.start(st);
        if (mesh.set()) launch_inspect_mesh_tick(cam, scene, mesh.dev, sigma, ctl, dev, (int)B, m, x, y, res, st);
        else launch_inspect_tick(cam, scene, sigma, ctl, dev, (int)B, m, x, y, res, st);
        (void)rtimer.stop(st);
        (void)timer.stop(st);
    }
};

}  // namespace brov
