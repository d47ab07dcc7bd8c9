// nmpc_device.hpp -- device-side parameter block and HBM layout shared by the kernels and the host API.
#pragma once
#include <string>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bluerov2_nmpc.h"

namespace brov {

// HBM layout (all FP64, instance-major; "tile" = 16x16 doubles stored row-major = MFMA C/D register image,
// see qp_kernel.hip):
//   x0    [B][12]             yref [B][N+1][16] or shared [N+1][16]        par [B][N+1][16]
//   x     [B][N+1][12]        u    [B][N][4]      pi [B][N][12]            lam [B][N][8]
//   BA    [B][N][12][16]      row k, col c:  d x+_k / d (x,u)_c            (3/4 tile: rows 0..11)
//   bvec  [B][N][12]          phi(x_i,u_i) - x_{i+1}
//   kktp  [B][N]              per-interval partial of the NLP KKT inf-norm
//   Riccati by-products per stage:  Ks [B][N][4][16] (gain, row m, col c), Kt [B][N][12][16] (gain^T, row c, col m),
//                                   Mt [B][N][4][16] (Huu^-1, cols 0..3), Pb [B][N][12], kff [B][N][4]
//   IPM state per instance:         ipm [B][IPM_NARR][N*4]
struct DevParams {
    int32_t B, N;
    int32_t qp_iter_max, early_exit;
    int32_t pit;             // parallel-in-time step-0 solve ahead of the resident windowed kernel: 0 off, 1 instances whose previous step was an early exit, 2 every instance (tests)
    int32_t pit_light;       // ... tries whose pins sit below the first segment's checkpoint reuse the step-0 pass (default 1; BROV_PIT_LIGHT=0: A/B, tests)
    int32_t pit_try;         // ... and, when the step-0 answer leaves the box, ONE active-set try parallel in time as well (default 1; BROV_PIT_TRY=0: A/B)
    int32_t pit_blocks;      // blocks of rti_pit_kernel = tickets it serves (win_blocks; B where every instance has a workspace of its own: pit_rounds_stages)
    int32_t* pit_done;       // [B]: rti_pit_kernel has completed the instance's step (the resident kernel behind it skips it); nullptr when pit = 0
    double robust_kkt_max;   // robust pivot form on demand only while the entering KKT is at most this (1e6; BROV_ROBUST_KKT_MAX: development knob)
    int32_t partial_refactor, robust_pivot;   // robust_pivot: ill-conditioned instances refactorise in the Cholesky pivot form (default 1; BROV_ROBUST_PIVOT=0: A/B);   // active-set tries restart their factor sweep from the step-0 checkpoint where they may (default 1; BROV_PARTIAL_REFACTOR=0: A/B)
    int32_t rti_split;       // resident windowed kernel, rti_phase 1 / 2 as separate launches: 1 = preparation (linearise + step-0 factor sweep, LDS image parked per instance), 2 = feedback (image fetched, everything that depends on x0); 0 = one launch
    int32_t on_failure, dump_lin;   // BROV_ON_FAILURE_*; dump_lin != 0: LDS-resident kernels copy [A B | b] out to BA / bvec (tests)
    double Ts, tol_mu, tol_stat;
    double W[16], We[12], lbu[4], ubu[4];
    // inputs
    const double* x0;
    const double* yref;
    int64_t yref_stride;  // doubles between instances (0 when one window is shared)
    const double* par;    // always [B][N+1][16]
    const double* par_rp; // 6-disturbance model variant: roll / pitch disturbance moments [B][N+1][2]; nullptr = the shipped model
    // iterate
    double* x;
    double* u;
    double* pi;
    double* lam;
    // linearisation
    double* BA;
    double* bvec;
    double* kktp;
    // Riccati storage
    double* Ks;
    double* Kt;
    double* Mt;
    double* Pb;
    double* kff;
    double* vhat;   // [B][N][4] candidate inputs of the current Newton solve
    double* ipm;    // [B][IPM_NARR][N*4]
    double* dxb;    // [B][N+1][12] QP primal step of the states
    const double* cst;  // [W16 | We12 pad4 | lbu4 | ubu4]
    // general grid (streaming kernels only; both nullptr = uniform step Ts and one stage weight): tsv [N] time steps = ERK4 step and
    // cost scaling per stage (acados_solver_bluerov2.c:111-131), wst [N+1][16] = the scaled weights per stage, ts_i * (i == 0 ? W_0 : W),
    // row N = [We | 0] (separate stage-0 weight: :422-441)
    const double* tsv;
    const double* wst;
    brov_result* res;
    // host mailbox (brov_tick_host, small batches): the record additionally goes straight into pinned host memory, followed by the
    // instance's sequence word -- the host polls that word instead of waiting for a copy and a stream synchronisation
    brov_result* mail;
    int32_t* mail_flag;
    int32_t mail_seq;
    int32_t mail_early;      // resident windowed kernel: send the record ahead of the last adjoint sweep when the answer needs none of it
    // windowed kernel (N >= 24): per-block parking image + scratch, instance hand-out counter, stages per window
    double* ws;
    int64_t ws_stride;   // doubles per block
    int32_t* counter;        // this launch's hand-out counter (zero on entry) ...
    int32_t* counter_next;   // ... and the next launch's, which block 0 of this launch zeroes (no memset node between the launches)
    int32_t win_L, win_blocks;
    // work ordering (qp_kernel.hip, sched_map): three rotating buffers of [64 class counters | class lists | pos[B]] int32 -- the
    // instances whose QP had active bounds in the previous solve are handed out first in this one; nullptr = instances in index order
    int32_t* sched;
    int32_t sched_stride, sched_r, sched_w, sched_z;   // buffer read / written / zeroed by this launch
    // rti_fused_kernel_ticks (brov_solve_ticks): `ticks` RTI steps of an instance back to back inside one launch; the shared reference window
    // moves on tick_yref doubles per step (row stride x 16 inside the resident trajectory table; 0: the window stays); optional status log
    int32_t ticks;
    int64_t tick_yref;
    int32_t* tick_status;    // [ticks][B] or nullptr
    // ... and, for brov_closed_loop, the plant update behind every step: x0 <- ERK4(x0, u0 of the step, plant parameters) (nullptr: no plant, x0 held)
    const double* plant_pp;  // [B][16] true plant parameters
    const double* plant_rp;  // 6-disturbance variant: roll / pitch moments, instance b at plant_rp + b * plant_rp_stride (or nullptr)
    int32_t plant_rp_stride, plant_substeps;
    double plant_dt;
    double* x0_rw;           // = x0, writable
    double* plant_xlog;      // [ticks][B][12] states after every step, or nullptr
    double* plant_ulog;      // [ticks][B][4] applied inputs, or nullptr
    unsigned long long* dbg;  // optional per-instance phase timestamps (s_memtime), 8 slots per instance; nullptr = off
};

// development knobs (BROV_* environment variables), read once per solver by the host API (nmpc_api.hip, read_knobs)
struct DevKnobs {
    double robust_kkt_max = 1e6;
    int robust_pivot = 1, partial_refactor = 1, mail_early = 1, split_resident = 1, pit = 1, split_parallel = 1, pit_try = 1, pit_light = 1;
    int tick_mailbox = 1, tick_bulk = 1, tick_zerocopy = 1, sched = 1, force_windowed = 0, fused_waves = 0, lds_pad = 0, tick_breakdown = 0, closed_loop_fused = 1;
    int no_resident = 0, win_blocks = 0, pit_rounds = 1;   // size the workspaces: in force as read at create (win_blocks 0: as many as fit)
    int win_long = 0;                                      // the long-horizon windowed instantiations at every horizon (A/B)
};

enum { IPM_V = 0, IPM_TL, IPM_TU, IPM_LL, IPM_LU, IPM_GAM, IPM_RT, IPM_DVA, IPM_ACT, IPM_NARR };

// qp_kernel.hip: the kernel table, the choice of a kernel from a call's properties, and the launches.  The launchers read the variant
// from what the host's plan left in P (tsv, ticks, rti_split, win_L, pit && pit_done, mail && mail_early).
int sched_buffer_ints_host(int B);   // int32 per work-ordering buffer (three of them)
int prepare_kernels_on_device(std::string* why);   // dynamic-LDS limits of every solver kernel on the CURRENT device, once per device, checked (brov_create)
void launch_linearise(const DevParams& P, hipStream_t st);   // streaming pair: linearisation into HBM ...
void launch_qp(const DevParams& P, hipStream_t st);          // ... and the QP out of it
void launch_fused(const DevParams& P, hipStream_t st, const DevKnobs& k);   // linearise + QP in one kernel, stage blocks in LDS; P.ticks steps per instance in one launch
bool fused_supported(int N);      // whole horizon fits the LDS slice (N <= 23)
// windowed LDS-resident kernel for longer horizons: persistent blocks (one wavefront each) that take instances from a counter
void launch_windowed(const DevParams& P, hipStream_t st, const DevKnobs& k);
void lds_kernel_info(int N, int win_L, bool windowed, int32_t info[4], const DevKnobs& k);   // LDS bytes per block, blocks per CU, threads, kernel kind
bool pit_supported(int N, int win_L);       // rti_pit_kernel ahead of the resident kernel
bool windowed_is_resident(int win_L);      // one window = the whole horizon (small batches)
int windowed_stage_count(int N, int B, int cus, const DevKnobs& k);   // stages per window (= N for batches of at most one instance per CU: resident mode)
int windowed_blocks(int B, int L, int cus, const DevKnobs& k);        // persistent blocks of a launch on the current device
size_t windowed_ws_doubles(int N, int L); // per-block workspace
bool split_resident_horizon(int N);           // rti_phase 1 / 2 on the resident kernel's split launches at a fused-kernel horizon
int pit_rounds_stages(int N, int B, int cus, const DevKnobs& k);      // batches of up to two instances per CU: resident stage count for parallel-in-time rounds, or 0
void launch_window(const double* traj, int rows, const int* lines, int line0, int B, int N, int ncols, double* out, hipStream_t st);
void launch_plant(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, int B, double dt, int substeps,
                  double* xlog, double* ulog, hipStream_t st);   // prp: roll / pitch disturbance moments, instance b at prp + b * rp_stride (or nullptr)
void launch_candidates(int kind, const double* p0, const double* p1, const double* phase, double t0, double dt, int B, int N,
                       double* out, hipStream_t st);

// time-varying world-frame wrench of the plant (plant_wrench.hip; include/bluerov2_nmpc.h, brov_plant_wrench_*): the generator's data.
// A pure function of (this record, instance, tick): nothing of it lives on the device between two launches.
struct WrenchGen {
    int mode = 0;                    // BROV_WRENCH_*
    int rows = 0;                    // table mode
    const double* w = nullptr;       // constant mode: [B][6]
    const double* tab = nullptr;     // table mode: [rows][6], shared by the batch
    const double* gain = nullptr;    // table mode: [B] or nullptr
    unsigned long long seed = 0;     // periodic mode
    double scale = 6.0, phase0 = 0.0, dphi = 0.125, tz_div = 3.0;
};
void launch_plant_wrench(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, int B, double dt, int substeps,
                         double* xlog, double* ulog, const WrenchGen& g, long long tick, double* wlog /*[B][6] or nullptr*/, hipStream_t st);
void launch_wrench_eval(const WrenchGen& g, int B, long long tick, double* out /*[B][6]*/, hipStream_t st);
void launch_gather_cols(const double* src, int B, int src_stride, int col0, int ncols, double* dst /*[B][ncols]*/, hipStream_t st);

// thruster stage of the plant (plant_wrench.hip; include/bluerov2_nmpc.h, brov_thruster_*): between the six commands of the result record and
// the body wrench the model integrates.  A pure function of (these records, instance, tick): the stage keeps no state.
struct ThrusterPar {              // shared by the batch and wave-uniform: passed by value in the kernel arguments
    double K[36];                 // [6][6] rows = generalised force axes [X Y Z K M N], columns = thrusters
    double lo[6], hi[6];          // limits of the commands, always applied
};
struct ThrusterDev {              // per instance
    const double* gain = nullptr;        // [B][6]
    const double* bias = nullptr;        // [B][6]
    const long long* onset = nullptr;    // [B]: gain and bias apply from this tick on
    int32_t* clip_ticks = nullptr;       // [B][6] statistics of the plant steps ...
    double* lost_sq = nullptr;           // [B]
    double* last = nullptr;              // [B][6] ... and the thrusts the last one applied
};
void launch_plant_thruster(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, int B, double dt, int substeps,
                           double* xlog, double* ulog, const ThrusterPar& T, const ThrusterDev& D, const WrenchGen& g, long long tick,
                           double* wlog /*[B][6] or nullptr*/, hipStream_t st);   // g.mode OFF: the instantiation without a world wrench
void launch_thruster_eval(const ThrusterPar& T, const ThrusterDev& D, int B, long long tick, const double* commanded /*[B][6]*/,
                          double* applied /*[B][6]*/, double* wrench /*[B][6]*/, hipStream_t st);

// ocean current on the plant (plant_current.hip; include/bluerov2_nmpc.h, brov_current_*): a world-frame water velocity per instance and tick.
// CONSTANT / TABLE: a pure function of (this record, instance, tick).  GAUSS_MARKOV: the device state c, which every plant step advances.
struct CurrentGen {
    int mode = 0;                    // BROV_CURRENT_*
    int rows = 0;                    // table mode
    const double* v = nullptr;       // constant mode: [B][3]
    const double* tab = nullptr;     // table mode: [rows][3], shared by the batch
    const double* gain = nullptr;    // table mode: [B] or nullptr
    double* c = nullptr;             // Gauss-Markov mode: [B][3] the state, what the next step applies
    const double* mean = nullptr;    // Gauss-Markov mode: [B][3]
    unsigned long long seed = 0;
    double mu[3] = {0, 0, 0}, amp[3] = {0, 0, 0}, lo[3] = {-5, -5, -5}, hi[3] = {5, 5, 5};   // per world axis, shared by the batch
    double step = 0.0;               // seconds per tick
    double* last = nullptr;          // [B][3] the current the last plant step applied
};
// one plant step under the current of `cg` at `tick` (mode not OFF): behind the thruster stage where th_on, under the world wrench of g where
// its mode is not OFF; statistics and logs as launch_plant_thruster / launch_plant_wrench leave them; Gauss-Markov mode: the state advances
void launch_plant_current(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, int B, double dt, int substeps,
                          double* xlog, double* ulog, bool th_on, const ThrusterPar& T, const ThrusterDev& D, const WrenchGen& g, const CurrentGen& cg,
                          long long tick, double* wlog /*[B][6] or nullptr*/, hipStream_t st);
void launch_current_eval(const CurrentGen& cg, int B, long long tick, double* out /*[B][3]*/, hipStream_t st);

// Coriolis stage of the plant (plant_coriolis.hip; include/bluerov2_nmpc.h, brov_coriolis_*): the rigid-body and added-mass Coriolis forces on
// rows X, Y, Z, N, a pure function of (this record, the instance's plant parameters, its state, the water's velocity).  No state.
struct CoriolisGen {
    int terms = 0;                   // BROV_CORIOLIS_* bit mask, 0: off
    double ka = 0.0, ma = 1.2481;    // roll / pitch added inertia, shared by the batch
    double* last = nullptr;          // [B][4] the force at the start state of the last plant step under the stage
};
// one plant step under the stage (terms not 0): launch_plant_current's step -- behind the thruster stage where th_on, under the world wrench
// of g where its mode is not OFF and in the current of cg, which may be OFF here -- with the stage's force at every RK stage; co.last <- the force at the start
void launch_plant_coriolis(double* x0, const brov_result* res, const double* pplant, const double* prp, int rp_stride, int B, double dt, int substeps,
                           double* xlog, double* ulog, bool th_on, const ThrusterPar& T, const ThrusterDev& D, const WrenchGen& g, const CurrentGen& cg,
                           const CoriolisGen& co, long long tick, double* wlog /*[B][6] or nullptr*/, hipStream_t st);
// the force alone: out [B][4] for the states x [B][12] in water moving with vc [B][3] (nullptr: still), added masses from pplant [B][16]
void launch_coriolis_eval(const CoriolisGen& co, const double* pplant, int B, const double* x, const double* vc, double* out, hipStream_t st);

// sensor stage between the plant and the controller (sensor_kernel.hip; include/bluerov2_nmpc.h, brov_sensor_*): the measured state the
// solve, the observer and the estimator read in place of the plant's true state.  A fresh sample is a pure function of (these records,
// instance, measurement index, channel, true value); the only state is the measured state itself, which a held channel keeps.
struct SensorPar {                // shared by the batch and wave-uniform: passed by value in the kernel arguments
    double quant[12];             // quantisation step of a channel, 0: none
    int32_t period[12];           // a regular refresh samples channel c where index % period[c] == 0
    unsigned long long seed;
};
struct SensorDev {                // per instance
    const double* sigma = nullptr;       // [B][12] standard deviation of the noise
    const double* bias = nullptr;        // [B][12]
    const double* dropout = nullptr;     // [B] probability that a regular refresh's fix is dropped
    int32_t* dropped = nullptr;          // [B] statistics of the regular refreshes: fixes dropped ...
    double* err_sq = nullptr;            // [B][12] ... and the running sum of (measured - true)^2 behind each of them
};
// one refresh of ymeas [B][12] from the true state x [B][12] at measurement index m (0 <= m < 2^24): regular (periods, dropout, statistics)
// or forced (every channel fresh, no dropout draw, statistics untouched)
void launch_sensor_measure(const SensorPar& P, const SensorDev& D, int B, long long m, bool forced, const double* x, double* ymeas, hipStream_t st);
// the stage alone: fresh samples y [B][12] of the states x [B][12] at index m and the dropout verdicts [B]; moves nothing
void launch_sensor_eval(const SensorPar& P, const SensorDev& D, int B, long long m, const double* x, double* y, int32_t* dropped, hipStream_t st);

// IMU/GPS stage of the plant (imu_kernel.hip; include/bluerov2_nmpc_imu.h, brov_imu_*): what the error-state filter reads, made from the TRUE state
struct ImuPar {                   // shared by the batch and wave-uniform: passed by value in the kernel arguments
    double h, g;                  // the plant step the stage follows; gravity
    int32_t gps_every, flags;     // a fix is due where index % gps_every == 0; BROV_IMU_*
    unsigned long long seed;
};
struct ImuDev {                   // per instance
    const double* sigma = nullptr;       // [B][12] accelerometer, gyro, GPS position, attitude
    const double* bias = nullptr;        // [B][6] accelerometer, gyro
    const double* dropout = nullptr;     // [B] probability that a due fix is dropped
    double* vprev = nullptr;             // [B][3] v_I of the last sample
    double* plast = nullptr;             // [B][3] gps_p of the last fix
    int32_t* mlast = nullptr;            // [B] its index
    int32_t* stats = nullptr;            // [B][3] samples, fixes taken, fixes dropped of the regular refreshes
};
struct ImuOut { double *imu, *gps_p, *gps_v, *qm; int32_t* fix; };   // [B][6], [B][3], [B][3], [B][4], [B]
// one refresh from the true state x at index m, regular or forced (imu_measure_kernel)
void launch_imu_measure(const ImuPar& P, const ImuDev& D, const ImuOut& O, int B, long long m, bool forced, const double* x, hipStream_t st);
// the stage alone for given x, v_prev [B][3], gps_p_last [B][3], m_last [B] at index m; moves nothing
void launch_imu_eval(const ImuPar& P, const ImuDev& D, const ImuOut& O, int B, long long m, const double* x, const double* vprev, const double* plast,
                     const int32_t* mlast, hipStream_t st);

// range stage and inspection controller (inspect_kernel.hip; include/bluerov2_nmpc_inspect.h, brov_range_*, brov_inspect_*)
struct RangeScene {               // shared by the batch and wave-uniform: passed by value in the kernel arguments, read with scalar loads
    double lo[BROV_RANGE_MAX_BOXES][3], hi[BROV_RANGE_MAX_BOXES][3];
    int32_t n;
};
struct InspectDev {               // per instance
    brov_inspect_state* state = nullptr;   // [B]
    brov_inspect_stats* stats = nullptr;   // [B]
    double* range = nullptr;               // [B] the last range
    int32_t* status = nullptr;             // [B] the mission status behind the last tick
};
// the range stage alone for the states x [B][12] at index m: range [B], hits [B], rot [B][9] or nullptr, depth [B][roi * roi] or nullptr
void launch_range_eval(const brov_range_params& P, const RangeScene& S, const double* sigma, int B, long long m, const double* x, double* range,
                       int32_t* hits, double* rot, double* depth, hipStream_t st);
// the controller alone: one tick from state_in on range, z, psi [B] into state_out and rec; stats [B] in and out, or nullptr
void launch_inspect_eval(const brov_inspect_params& C, int B, const brov_inspect_state* state_in, const double* range, const double* z,
                         const double* psi, brov_inspect_state* state_out, brov_result* rec, brov_inspect_stats* stats, hipStream_t st);
// one tick of the loop: rays from the true state x at index m, the controller on z and psi of y (what the controller sees), the record into res
void launch_inspect_tick(const brov_range_params& P, const RangeScene& S, const double* sigma, const brov_inspect_params& C, const InspectDev& D,
                         int B, long long m, const double* x, const double* y, brov_result* res, hipStream_t st);

// delay stage of the plant (delay_kernel.hip; include/bluerov2_nmpc.h, brov_delay_*): a ring [B][D][10] of the last D commanded records
// (u0[4] | thrust[6]), indexed by the stage's own step count n.
// step n of the stage: applied[b] = res[b] with u0 and thrust of step n - delay[b] (zeros before the first), res[b]'s own into slot n mod D;
// ulog: [B][4] the COMMANDED u0, or nullptr.  The host has checked 0 <= delay[b] <= D - 1
void launch_delay_shift(const brov_result* res, brov_result* applied, const int32_t* delay, double* ring, int D, long long n, int B, double* ulog,
                        hipStream_t st);
// xhat [B][12] = y [B][12] carried through the u0 of steps n - comp ... n - 1 (comp <= D - 1) by one ERK4 step over dt_pred each, with the
// parameters of instance b at par + b * par_stride and its roll / pitch moments at prp + b * rp_stride (or nullptr)
void launch_delay_predict(const double* y, const double* par, int par_stride, const double* prp, int rp_stride, const double* ring, int D, long long n,
                          int comp, double dt_pred, double* xhat, int B, hipStream_t st);

// rotor stage of the plant (rotor_kernel.hip; include/bluerov2_nmpc.h, brov_rotor_*): first-order dynamics of the six thrusters between the
// commands and the plant, behind the delay stage and ahead of the thruster stage.  The only state is r [B][6].
struct RotorPar {                 // shared by the batch and wave-uniform: passed by value in the kernel arguments
    double lo[6], hi[6];          // limits of the commands ahead of the dynamics
};
// one step of the stage: applied[b] = rec[b] with thrust = the mean thrusts m over the step and u0 = the allocation's left inverse of m; the
// state advances, last [B][6] = m, lag_sq [B] += |c - m|^2; alpha, beta: [B][6] from the host; ulog: [B][4] the COMMANDED u0, or nullptr
void launch_rotor_shift(const brov_result* rec, brov_result* applied, const RotorPar& P, const double* alpha, const double* beta, double* state,
                        double* last, double* lag_sq, int B, double* ulog, hipStream_t st);
// the stage alone: applied [B][6] and state_out [B][6] for the commands commanded [B][6] from the state state [B][6]; moves nothing
void launch_rotor_eval(const RotorPar& P, const double* alpha, const double* beta, const double* commanded, const double* state, double* applied,
                       double* state_out, int B, hipStream_t st);

// thrust-curve stage of the plant (curve_kernel.hip; include/bluerov2_nmpc_curve.h, brov_curve_*): the COMMAND part (pre-map, quantisation)
// ahead of the rotor stage and the THRUST part (conversion curve, efficiency) behind it; with the rotor stage off both in one launch
enum { CURVE_COMMAND = 1, CURVE_THRUST = 2, CURVE_BOTH = 3 };   // the parts a launch runs: the values of BROV_CURVE_PART_*
struct CurvePar {                 // shared by the batch and wave-uniform: passed by value in the kernel arguments
    int32_t kind, pre;            // BROV_CURVE_* / BROV_CURVE_PRE_*
    int32_t Kc, Kp;               // knots of the curve table and of the pre table (0: none set)
    int32_t amps, reserved_;      // the curve table carries the amps column
    double quantum, inv_quantum, k, kl, kr, dl, dr;
    double pre_poly[5];           // highest degree first
};
// a table as the kernels stage it in LDS, Ke = K rounded up to even so that every part starts on 16 bytes:
//   x [Ke] | (y, slope) [K] pairs | (amps, amps_slope) [K] pairs, the last only with an amps column
__host__ __device__ inline int curve_image_doubles(int K, bool amps) { return K <= 0 ? 0 : ((K + 1) & ~1) + 2 * K + (amps ? 2 * K : 0); }
struct CurveBooks {               // [B][6] wanted, last_command, last_thrust, dead_ticks; [B] err_sq, charge
    double *wanted, *last_command, *last_thrust, *err_sq, *charge;
    int32_t* dead_ticks;
};
// one step of the part(s) `part`: applied[b] = rec[b] with thrust = the part's output and, where a bit of the six changed, u0 = the
// allocation's left inverse of it.  COMMAND stores wanted and last_command; THRUST reads wanted, stores last_thrust and keeps err_sq,
// dead_ticks and charge (dt: the plant step's); BOTH does both.  eff: [B][6]; img_curve / img_pre: the table images; ulog: [B][4] the
// COMMANDED u0, or nullptr
void launch_curve_shift(int part, const brov_result* rec, brov_result* applied, const CurvePar& P, const double* eff, const double* img_curve,
                        const double* img_pre, const CurveBooks& bk, double dt, int B, double* ulog, hipStream_t st);
// the part(s) alone: out [B][6] and amps_out [B][6] (zeros without an amps column or a THRUST part) for in [B][6]; moves nothing
void launch_curve_eval(int part, const CurvePar& P, const double* eff, const double* img_curve, const double* img_pre, const double* in, double* out,
                       double* amps_out, int B, hipStream_t st);

}  // namespace brov
