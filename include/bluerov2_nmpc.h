/*
 * bluerov2_nmpc.h -- C ABI of the MI355X-native batched BlueROV2 NMPC (SQP real-time-iteration) solver.
 *
 * One handle owns B independent OCP instances (12 states / 4 inputs / 16 parameters, N shooting intervals) resident
 * in the HBM of ONE GPU.  brov_solve() performs, for every instance, exactly what ONE call of the reference's
 *     bluerov2_acados_solve(capsule)      bluerov2_dobmpc/scripts/c_generated_code/acados_solver_bluerov2.c:945-951
 * performs for its single instance (ocp_nlp_solve with SQP_RTI: ERK4+sensitivities, Gauss-Newton LS cost, box QP,
 * full step), and the setters replace the per-tick acados calls of the callers:
 *     brov_set_x0      <- ocp_nlp_constraints_model_set(..,0,"lbx"/"ubx",x0)   bluerov2_dob.cpp:320-321, ctrller/mpc.cpp:121-137
 *     brov_set_params  <- bluerov2_acados_update_params(capsule,i,p,16)         bluerov2_dob.cpp:324-355, acados_solver_bluerov2.c:835-883
 *     brov_set_yref    <- ocp_nlp_cost_model_set(..,i,"yref",yref[i])           bluerov2_dob.cpp:370-372, ctrller/mpc.cpp:46-58
 *     brov_get_u0      <- ocp_nlp_out_get(..,0,"u",u0)                          bluerov2_dob.cpp:388
 *     brov_get_results <- status / nlp_out->inf_norm_res / "time_tot"           bluerov2_dob.cpp:377-386
 *     brov_set/get_iterate <- ocp_nlp_out_set/get(..,"x"/"u")                   main_bluerov2.c:211-247
 *     brov_reset       <- bluerov2_acados_reset                                 acados_solver_bluerov2.c:797-830
 * The batch=1 acados-shaped shim (include/acados_shim/, libacados_ocp_solver_bluerov2.so) is a veneer over this API.
 *
 * Plain C: pointers + sizes, no C++/torch types.  Every pointer argument is tagged HOST or DEVICE below; DEVICE
 * pointers must be valid on the handle's GPU.  All calls on one handle must come from one thread at a time
 * (same contract as an acados capsule).  Layouts are instance-major, row-major, FP64:
 *     x0   [B][12]            yref [B][N+1][16] (or shared [N+1][16])      p [B][16] or [B][N+1][16]
 *     x    [B][N+1][12]       u    [B][N][4]      pi [B][N][12]            lam [B][N][8] = [lower4 | upper4]
 * There is no CPU fallback: every entry point that needs the GPU returns BROV_ERR_NO_DEVICE when none is usable.
 */
#ifndef BLUEROV2_NMPC_H_
#define BLUEROV2_NMPC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BROV_NX 12
#define BROV_NU 4
#define BROV_NP 16
#define BROV_NY 16

/* error codes of the API itself (solver status per instance uses the acados codes below) */
#define BROV_OK 0
#define BROV_ERR_ARG -1
#define BROV_ERR_NO_DEVICE -2
#define BROV_ERR_HIP -3
#define BROV_ERR_ALLOC -4

/* per-instance solver status == acados return codes (acados/utils/types.h as used by the callers) */
#define BROV_STATUS_SUCCESS 0
#define BROV_STATUS_NAN 1
#define BROV_STATUS_MAXITER 2
#define BROV_STATUS_MINSTEP 3
#define BROV_STATUS_QP_FAILURE 4

/* options; brov_default_opts() fills the values baked into the reference's generated solver
 * (acados_solver_bluerov2.c: W :422-481, bounds :559-566, qp_iter_max :668, Ts :389) */
typedef struct brov_opts {
    int32_t N;              /* shooting intervals, 1..BROV_MAX_N */
    int32_t qp_iter_max;    /* 50 */
    double  Ts;             /* uniform interval length [s]; cost scaling of stages 0..N-1 */
    double  W[BROV_NY];     /* diagonal stage weight on y = [x;u] */
    double  We[BROV_NX];    /* diagonal terminal weight */
    double  lbu[BROV_NU];
    double  ubu[BROV_NU];
    double  qp_tol_mu;      /* interior point, bound resolution (1e-7): at termination every input is within this distance of a bound or
                             * the bound's multiplier divided by the input's weight is below it */
    double  qp_tol_stat;    /* interior point, stationarity target (1e-9, tracked residual, absolute) */
    int32_t qp_early_exit;  /* 1: accept the equality-constrained minimiser when it satisfies the bounds (exact) */
    int32_t kernel_path;    /* BROV_PATH_AUTO (LDS-resident kernels: whole horizon for N <= 23, windowed above), _STREAMING, _FUSED */
    int32_t on_failure;     /* what happens to an instance whose step fails (status NAN / MINSTEP / QP_FAILURE):
                             *   BROV_ON_FAILURE_KEEP    iterate left untouched -- what acados' SQP_RTI does (it returns before
                             *                           update_variables); a diverged iterate then fails again every tick
                             *   BROV_ON_FAILURE_RESTART (default) cold restart at the measured state (if x0 is finite): x_i = x0 for all i, u = 0,
                             *                           multipliers 0, so that the instance can recover on the next tick
                             * In both cases the record's u0 is the last successfully computed input (zero-order hold), clamped
                             * to [lbu, ubu] with NaN -> 0: plant / thrust consumers never see a diverged input. */
    int32_t reserved_;
} brov_opts;

#define BROV_ON_FAILURE_KEEP 0
#define BROV_ON_FAILURE_RESTART 1

#define BROV_PATH_AUTO 0
#define BROV_PATH_STREAMING 1 /* lin_wave_kernel + qp_kernel, stage blocks streamed through HBM; any N <= BROV_MAX_N */
#define BROV_PATH_FUSED 2     /* one kernel, one wavefront per instance, stage blocks in LDS: the whole horizon (N <= 23) or a
                               * window of <= 20 stages at a time with the other windows parked in a per-instance HBM image */

#define BROV_PATH_WINDOWED 3  /* reported by brov_last_kernel_path only: the windowed flavour of BROV_PATH_FUSED / _AUTO (N >= 24) */

/* Longest horizon.  The reference's create_with_discretization takes any N (acados_solver_bluerov2.c:734-783).  Here the QP loop keeps the 4 N
 * inputs of an instance as elements per lane of its wavefront: 8 per lane as register copies in the LDS-resident kernels (N <= 128 =
 * BROV_MAX_N_LDS), 16 per lane read from HBM element by element beyond (N <= 256; round 5): the streaming pair and the large-batch windowed
 * kernel's long-horizon instantiations (rti_window_kernel_long, _long_grid, _long_ticks), which BROV_PATH_AUTO runs there.  N > 256 is refused by brov_create with BROV_ERR_ARG (the drop-in's create
 * returns non-zero).  (The reference ships N = 80.) */
#define BROV_MAX_N 256
#define BROV_MAX_N_LDS 128

/* 104-byte per-instance result record; this is also the record all-gathered across GPUs ("optimal
 * thrusts/costs for selection") */
typedef struct brov_result {
    double  u0[BROV_NU];    /* optimal first input after the step  (ocp_nlp_out_get(..,0,"u")) */
    double  cost;           /* NLS objective at the updated iterate */
    double  kkt;            /* NLP KKT inf-norm of the iterate entering the step (-> ocp_nlp_out::inf_norm_res) */
    int32_t status;         /* BROV_STATUS_* */
    int32_t qp_iter;        /* interior-point iterations used (0 = early exit) */
    double  thrust[6];      /* thrust allocation of u0, written by the solve kernel (bluerov2_dob.cpp:390-395) */
} brov_result;

typedef struct brov_solver brov_solver; /* opaque */

void brov_default_opts(brov_opts* o, int N, double Ts);

/* lifecycle.  device = HIP device ordinal.  Allocates all HBM state for B instances; initial iterate, yref, p and
 * x0 are the reference's create defaults (x_i=[0,0,-20,0..], u_i=0, yref=0, p=0; acados_solver_bluerov2.c:355-364,
 * 681-708). */
int  brov_create(brov_solver** out, int device, int B, const brov_opts* opts);
void brov_destroy(brov_solver* s);
int  brov_batch(const brov_solver* s);
int  brov_horizon(const brov_solver* s);
size_t brov_device_bytes(const brov_solver* s);
const char* brov_last_error(void);

/* inputs.  *_host variants copy from HOST memory (blocking on the solver's stream); *_device variants take DEVICE
 * pointers and enqueue a device-to-device copy on `stream` (NULL = default stream); no host sync. */
int brov_set_x0_host(brov_solver* s, const double* x0 /*[B][12]*/);
int brov_set_x0_device(brov_solver* s, const double* x0, void* stream);
/* shared != 0: one [N+1][16] window used by every instance; else per-instance [B][N+1][16] */
int brov_set_yref_host(brov_solver* s, const double* yref, int shared);
int brov_set_yref_device(brov_solver* s, const double* yref, int shared, void* stream);
/* per_stage == 0: p[B][16] applied to all stages (what every reference caller does); else p[B][N+1][16] */
int brov_set_params_host(brov_solver* s, const double* p, int per_stage);
int brov_set_params_device(brov_solver* s, const double* p, int per_stage, void* stream);
/* single-instance, single-stage setters (the shim's update_params / cost_model_set); stage in [0,N] */
int brov_set_param_stage_host(brov_solver* s, int instance, int stage, const double* p16);
int brov_set_yref_stage_host(brov_solver* s, int instance, int stage, const double* y, int ny);

/* ---- reference windows built on the device (the step before the path: bluerov2_path/src/bluerov2_path.cpp:79-118,
 * bluerov2_dobmpc/src/bluerov2_dob.cpp:218-265).  A trajectory table [rows][16] (the reference's txt format: x y z phi theta
 * psi u v w p q r u1..u4, one row per 0.05 s) is kept in HBM; node i of a window that starts at `line` is row
 * min(line + i, rows - 1).  ncols = 16 copies whole rows (DOB node), ncols = 12 leaves the input reference at zero (CTRL
 * node, ctrller/mpc.cpp:242-262). */
int brov_traj_set_host(brov_solver* s, const double* traj /*[rows][16]*/, int rows);
int brov_traj_rows(const brov_solver* s);
/* one shared window; with ncols = 16 and the window inside the table its rows are used where they lie (no copy, no kernel) */
int brov_set_yref_from_traj(brov_solver* s, int line, int ncols, void* stream);
int brov_set_yref_from_traj_lines_host(brov_solver* s, const int32_t* lines /*[B]*/, int ncols);     /* per instance      */
/* analytic per-instance candidate windows (bluerov2_path/config/traj/lemniscate.py:18-39, circle.py:22-56 evaluated at
 * t0 + i*dt with per-instance shape parameters and phase): kind 0 lemniscate (p0 = amplitude, p1 = frequency),
 * kind 1 circle (p0 = radius, p1 = speed) */
int brov_set_yref_candidates_host(brov_solver* s, int kind, const double* p0, const double* p1, const double* phase /*[B]*/,
                                  double t0, double dt);
/* the same in two steps for per-tick use: shape parameters uploaded once (HOST pointers), then one kernel per tick on `stream`
 * (no host traffic) that rebuilds every instance's window at t0 + i*dt */
int brov_set_candidate_params_host(brov_solver* s, int kind, const double* p0, const double* p1, const double* phase /*[B]*/);
int brov_set_yref_candidates(brov_solver* s, double t0, double dt, void* stream);
/* read back the reference windows currently in force, as [B][N+1][16] (shared windows are replicated) */
int brov_get_yref_host(brov_solver* s, double* yref);
/* read back the model parameters currently in force, [B][N+1][16] */
int brov_get_params_host(brov_solver* s, double* par);

/* ---- closed-loop roll-outs on the device (the step after the path): plant update + reference advance ------------------
 * Plant = the OCP's own 12-state model (bluerov2.py:103-137) integrated with ERK4 over one control period with u0 of the
 * last solve and per-instance TRUE parameters (Monte-Carlo disturbance draws / model mismatch); the thrusters see
 * bluerov2_dob.cpp:390-395's allocation of that u0 (brov_get_thrusts_host). */
/* Without brov_plant_set_params_host the plant uses the controller's own stage-0 parameters, re-read whenever they may have
 * changed (any brov_set_params_* call, brov_params_device() hand-out) */
int brov_plant_set_params_host(brov_solver* s, const double* p /*[B][16]*/);
int brov_plant_step(brov_solver* s, double dt, int substeps, void* stream);   /* x0 <- ERK4(x0, u0, p_plant, dt) */
/* `ticks` control ticks entirely on the device: window(line0 + k) -> RTI step -> plant step; like the nodes, the window
 * advances one trajectory row per tick (bluerov2_dob.cpp:367-368) and the iterate is not shifted.  Optional HOST logs:
 * u_log [ticks][B][4] (applied inputs), x_log [ticks+1][B][12] (plant state before the first and after every tick),
 * st_log [ticks][B] (solver status). */
int brov_closed_loop(brov_solver* s, int ticks, int line0, int ncols, double dt, int substeps, double* u_log, double* x_log,
                     int32_t* st_log);
int brov_get_x0_host(brov_solver* s, double* x0 /*[B][12]*/);

/* ---- time-varying WORLD-frame wrench on the plant: the disturbance scenarios of the reference's applyBodyWrench()
 * (bluerov2_dobmpc/src/bluerov2_dob.cpp:754-892; bluerov2_ampc.cpp:1050-1150 is the same code with a slower phase rate).  The plant
 * parameters above pose a disturbance that is constant in the BODY frame; the reference applies its wrench in the world frame (:879), so
 * that its body-frame image turns with the vehicle -- the case the disturbance observer exists for.  Per instance, [fx fy fz tx ty tz],
 * a pure function of (mode data, instance b, tick k): no generator state lives on the device, any tick can be evaluated again.
 *   BROV_WRENCH_OFF       (default) brov_plant_step launches the plant kernel it always launched: bit-identical to a solver that never
 *                         touched this API
 *   BROV_WRENCH_CONSTANT  w[B][6]; the reference's mode 1 is (10, 10, 10, 0, 0, 0) (:813-816)
 *   BROV_WRENCH_PERIODIC  (:776-795)  t_k = phase0 + k * dphi -- a PRODUCT, evaluated afresh for every tick; the reference accumulates
 *                         dis_time += dt * 2.5, a running sum whose rounding depends on its history --, dphi = 0.125 in the DOB node (dt * 2.5),
 *                         0.025 in the AMPC node;  j = floor(t_k / pi), which must stay below 2^22;  amplitude of channel c in {X = 0, Y = 1,
 *                         Z = 2, N = 3}: A_c = scale * (0.5 + 0.5 U), U = (z >> 11) * 2^-53, z = splitmix64_finalise(seed + (n + 1) *
 *                         0x9E3779B97F4A7C15), n = (b << 24) | (j << 2) | c -- redrawn every half period, in [scale / 2, scale) like the
 *                         reference's uniform(0.5, 1) * 6;  wrench = sin(t_k) * (A_X, A_Y, A_Z, 0, 0, A_Y / tz_div): the yaw torque uses the Y
 *                         amplitude as the reference does (:787; its N draw is made and never used).  Batches up to 2^24 instances draw
 *                         independent amplitudes.
 *   BROV_WRENCH_TABLE     (:869-873) a table [rows][6] resident in HBM and shared by the batch, row min(k, rows - 1) (the reference indexes
 *                         past the end; this clamps, like the trajectory table), times an optional per-instance gain[B]
 * With a mode in force the plant is plant_wrench_kernel: the same ERK4, the wrench held over the tick and projected into the body frame at
 * EVERY stage with that stage's attitude (f_b = R^T f_w, t_b = R^T t_w), added to dx, dy, dz, the roll / pitch moments and dn ahead of the
 * mass scaling.  The tick counter k counts plant steps: +1 in brov_plant_step and in every tick of brov_closed_loop / _ex / _dob, whatever
 * the mode; brov_plant_wrench_seek sets it.  The one-launch closed loop and the *_ticks kernels know no wrench: brov_closed_loop with a mode
 * in force takes its launch-per-tick branch. */
#define BROV_WRENCH_OFF 0
#define BROV_WRENCH_CONSTANT 1
#define BROV_WRENCH_PERIODIC 2
#define BROV_WRENCH_TABLE 3
int brov_plant_wrench_constant_host(brov_solver* s, const double* w /*[B][6]*/);
int brov_plant_wrench_periodic(brov_solver* s, uint64_t seed, double scale, double phase0, double dphi, double tz_div);
int brov_plant_wrench_table_host(brov_solver* s, const double* tab /*[rows][6]*/, int rows, const double* gain /*[B] or NULL*/);
int brov_plant_wrench_off(brov_solver* s);
int brov_plant_wrench_mode(const brov_solver* s);
int brov_plant_wrench_seek(brov_solver* s, int64_t tick);   /* tick >= 0 */
int64_t brov_plant_wrench_tick(const brov_solver* s);
/* the wrench of every instance at `tick`, from the device generator; moves neither the plant nor the tick counter (zeros while OFF) */
int brov_plant_wrench_eval_host(brov_solver* s, int64_t tick, double* w /*[B][6]*/);
/* brov_closed_loop with the applied wrench of every tick logged: w_log HOST [ticks][B][6] or NULL (zeros while OFF).  Like brov_closed_loop
 * it delivers its logs only when the whole loop succeeded: a call that returns an error leaves the caller's log arrays untouched, also for
 * the ticks that ran. */
int brov_closed_loop_ex(brov_solver* s, int ticks, int line0, int ncols, double dt, int substeps, double* u_log, double* x_log,
                        int32_t* st_log, double* w_log);

/* ---- thruster stage of the plant: limits, per-instance faults and the propulsion matrix between the six thruster commands and the forces.
 * Without it every plant step gives the model exactly the wrench the controller asked for.  The vehicle does not: the reference's thruster
 * manager saturates at max_thrust 1540 (bluerov2_dobmpc/config/thruster_manager.yaml:7) while the OCP only boxes the four axes, and a weak,
 * stuck or dead thruster is the disturbance a disturbance observer exists for -- the observer is fed the COMMANDED thrusts, as in the
 * reference, so what the thrusters fail to deliver shows up as an estimated disturbance.  For instance b at plant tick k (the counter
 * brov_plant_wrench_tick reads), t = the six commands of the result record (brov_get_thrusts_host):
 *     c[i] = t[i] < lo[i] ? lo[i] : (t[i] > hi[i] ? hi[i] : t[i])                  a NaN passes through
 *     a[i] = k >= onset[b] ? gain[b][i] * c[i] + bias[b][i] : c[i]                 product rounded, then the sum rounded: no FMA
 *     g[r] = ((((K[r][0]*a[0] + K[r][1]*a[1]) + K[r][2]*a[2]) + K[r][3]*a[3]) + K[r][4]*a[4]) + K[r][5]*a[5]      every operation rounded
 * g = the body wrench [X Y Z K M N] the model integrates in place of the allocation of u0; the roll / pitch moments of the 6-disturbance
 * variant are added to g[3], g[4].  K is [6][6] row-major, rows = generalised force axes, columns = thrusters (the layout of the reference's
 * config/TAM.yaml); the default is the model's own (bluerov2.py:95-100, rows 3 and 4 zero).  Limits are shared by the batch and always apply;
 * gain, bias and onset are per instance and apply from the onset tick on: a weak thruster is gain 0.5, a dead one gain 0, a stuck one gain 0
 * and bias c.  The stage keeps no state (no thruster lag): a pure function of (data, instance, tick), bit-reproducible.
 * With the stage on, brov_plant_step and every loop built on it (brov_closed_loop / _ex / _dob / _track) launch plant_thruster_kernel, with the
 * wrench mode in force on top; the one-launch closed loop knows no thrusters, so the loops take their launch-per-tick branch; the u log stays
 * the commanded input; a brov_fleet refuses such a solver.  Each such plant step also keeps, per instance: clip_ticks[b][i] += (t[i] outside
 * [lo[i], hi[i]]), lost_sq[b] += sum_i (t[i] - a[i])^2 (six squares summed in index order, one add into the sum), and the applied thrusts a.
 * Refused with BROV_ERR_ARG and a text in brov_last_error() that starts with the call's name (nothing changes, nothing is waited for): a NULL
 * handle, lo[i] > hi[i], a NaN limit, a non-finite K, gain or bias, a negative onset or tick. */
void brov_thruster_default_matrix(double K[36]);
int brov_thruster_set_host(brov_solver* s, const double* K /*[6][6]; NULL: the model's*/, const double* lo /*[6]; NULL: -inf*/,
                           const double* hi /*[6]; NULL: +inf*/, const double* gain /*[B][6]; NULL: 1*/,
                           const double* bias /*[B][6]; NULL: 0*/, const int64_t* onset /*[B]; NULL: 0*/);   /* switches the stage on, resets the statistics */
int brov_thruster_off(brov_solver* s);                                /* the plant kernels as they always were; the statistics stay readable */
int brov_thruster_enabled(const brov_solver* s);                      /* 0 for NULL */
/* the stage alone at `tick`: moves neither the plant nor a counter nor a statistic (before any brov_thruster_set_host: the defaults) */
int brov_thruster_eval_host(brov_solver* s, int64_t tick, const double* commanded /*[B][6]*/, double* applied /*[B][6]*/, double* wrench /*[B][6]*/);
int brov_thruster_last_host(brov_solver* s, double* applied /*[B][6]*/);          /* of the last plant step behind the stage */
int brov_thruster_get_stats_host(brov_solver* s, int32_t* clip_ticks /*[B][6]*/, double* lost_sq /*[B]*/, int64_t* steps /*any NULL*/);
int brov_thruster_reset_stats(brov_solver* s);
int brov_thruster_last_seconds(brov_solver* s, double* seconds);                  /* the plant kernel's last launch behind the stage, HIP events */

/* ---- delay stage between the controller's commands and the plant, and a controller that predicts through it.  Without it the command solved
 * at tick k acts on the vehicle at tick k.  No real loop is like that: the input is applied after the solve, the transport to the thruster
 * manager and the ESCs.  With the stage on, every plant step (brov_plant_step and every tick of brov_closed_loop / _ex / _dob / _track) is
 * given the record commanded delay[b] plant steps earlier.  Per instance the stage keeps a ring of the last D commanded records, u0[4] and
 * thrust[6], D = max(max_b delay[b], comp) + 1, zero-filled when the stage is set or reset and indexed by the stage's OWN step count n (plant
 * steps since it was set or reset; brov_plant_wrench_seek does not disturb it).  Step n, c(n) = the solver's record (brov_results_device):
 *     a(n) = delay[b] == 0 ? c(n) : (n < delay[b] ? 0 : c(n - delay[b]))          read first, then c(n) is written into slot n mod D
 * and the plant kernel in force -- whatever the wrench mode, the thruster stage, the current and the sensor stage make it -- reads u0 and thrust
 * of a(n) in place of c(n).  Copies only: bit-reproducible.  The u log and the tracker keep the COMMANDED input; the one-launch closed loop
 * and the *_ticks kernels know no delay, so the loops take their launch-per-tick branch; a brov_fleet refuses such a solver.
 * comp > 0 (one number for the batch: the controller is designed for one nominal delay, delay[b] sweeps the real one against it): ahead of every
 * solve that takes its initial state from the solver (brov_solve, brov_solve_phase phases 0 and 2, brov_solve_ticks, every closed loop) the
 * predictor computes, per instance,
 *     x^ = Phi(... Phi(Phi(y, c(n - comp)), c(n - comp + 1)) ..., c(n - 1))
 * Phi = one explicit RK4 step over dt_pred (one substep) of the controller's own model: its stage-0 parameters as they stand (a handed-off
 * disturbance estimate included) and, 6-disturbance variant, its roll / pitch moments; y = what the controller knows of the state (the measured
 * state while the sensor stage is on); the inputs are the u0 of the queue, oldest first, zeros for steps before the first.  The solve starts
 * from x^.  brov_tick_host with its own x0 is refused while comp > 0.  The closed loops start tick k's shared reference window at row
 * line0 + k + comp -- the OCP starts comp ticks ahead --; the tracker still scores the true state after tick k against row line0 + k + 1.
 * A caller who sets windows by hand (brov_set_yref_*, brov_set_yref_from_traj) shifts them by comp rows itself.
 * observer_applied != 0: brov_ekf_update_from_solver reads the thrusts of the APPLIED records a(n) in place of the commanded ones.
 * Stage off (the default, and after brov_delay_off): every launch is the one of a solver without the stage.
 * Out of scope: thruster lag and other dynamics acting on the delayed value, sensor latency, per-instance comp, a non-zero initial fill of
 * the queue, the fleet, the one-launch *_ticks kernels.
 * Refused with BROV_ERR_ARG and a text in brov_last_error() that starts with the call's name (nothing changes, nothing is waited for): a NULL
 * handle, a delay or comp outside [0, BROV_DELAY_MAX], a non-finite dt_pred. */
#define BROV_DELAY_MAX 8
int brov_delay_set_host(brov_solver* s, const int32_t* delay /*[B]; NULL: all 0*/, int32_t comp, double dt_pred /*<= 0: the options' Ts*/,
                        int32_t observer_applied);                    /* switches the stage on, zeroes the ring and the step count */
int brov_delay_off(brov_solver* s);
int brov_delay_enabled(const brov_solver* s);                         /* 0 for NULL */
int brov_delay_comp(const brov_solver* s);                            /* plant steps the solves predict ahead; 0 while off and for NULL */
int brov_delay_depth(const brov_solver* s);                           /* D of the last brov_delay_set_host (1 before any); 0 for NULL */
int brov_delay_reset(brov_solver* s);                                 /* zeroes the ring and the step count */
int brov_delay_last_host(brov_solver* s, double* u0_applied /*[B][4]*/, double* thrust_applied /*[B][6]*/);   /* a(n) of the last plant step; one may be NULL */
int brov_delay_queue_host(brov_solver* s, double* u0 /*[B][D][4]*/);  /* the u0 of the last D commanded records, oldest first */
/* the predictor alone, from y [B][12] (NULL: the controller's state) into xhat [B][12]; moves nothing */
int brov_delay_predict_host(brov_solver* s, const double* y, double* xhat);
int brov_delay_predicted_host(brov_solver* s, double* xhat /*[B][12]*/);   /* what the last solve started from (refused before a solve has predicted) */
int brov_delay_last_seconds(brov_solver* s, double* shift_s, double* predict_s);   /* last launch of either kernel, HIP events; one may be NULL */

/* ---- rotor stage between the commands and the plant: first-order dynamics of the six thrusters, r' = (c - r) / tau (the reference's vehicle:
 * FirstOrder, timeConstant 0.2 s, i.e. four ticks of 50 ms, with a command clamp ahead of the dynamics).  Without it a command becomes force in
 * the tick it is issued.  The chain is delay -> rotor -> thruster stage (clip / fault / K) -> model: with the stage on, every plant step
 * (brov_plant_step and every tick of brov_closed_loop / _ex / _dob / _track) runs rotor_shift_kernel behind the delay stage's shift and ahead
 * of the plant kernel in force, which reads the applied record in place of the one it was given.  Per instance b and thruster i, with the
 * state r (zero when the stage is set or reset), the command t = thrust[i] of the record received and the coefficients alpha, beta:
 *     c  = t < cmd_lo[i] ? cmd_lo[i] : (t > cmd_hi[i] ? cmd_hi[i] : t)
 *     if c is not finite: c = r                          (a non-finite command moves nothing and is never stored)
 *     d  = r + (-c);   m = c + beta * d;   r' = c + alpha * d            every operation rounded on its own
 * alpha = exp(-h / tau), beta = (1 - alpha) / (h / tau) from the exact solution over the step h, computed on the HOST (brov_rotor_coeffs) and
 * uploaded.  m is the MEAN thrust over the step and what the plant is given under a zero-order hold: force enters the model linearly, so the
 * impulse of every step is exact.  tau = 0 has the pair (0, 0), and such a pair copies m = r' = c.  The applied record is the one received
 * with thrust = m and u0 = the allocation's left inverse of m (rc = the model's rotor constant):
 *     u0[0] = rc (-m0 - m1 + m2 + m3) / 4,  u0[1] = rc (m0 - m1 + m2 - m3) / 4,  u0[3] = rc (m0 - m1 - m2 + m3) / 4,  u0[2] = -rc (m4 + m5) / 2
 * (operation order: rotor_kernel.hip), so the plant without the thruster stage and the observer, which read u0, see the lagged forces.  An
 * instance whose six tau are 0 and whose commands pass unchanged (finite, inside the limits) has its whole record copied bit for bit.
 * Bit-reproducible against tests/rotor_restatement.py.  The u log and the tracker keep the COMMANDED input; the thruster stage's clip_ticks
 * and lost_sq count the lagged thrusts m as its "commanded".  Bookkeeping per step: last = m, lag_sq[b] += sum_i (c_i - m_i)^2, the stage's
 * own step count.  The coefficients hold for ONE step length: while the stage is on, brov_plant_step and every closed loop whose dt is not
 * bit-equal to h are refused with BROV_ERR_ARG and step nothing.  observer_applied != 0: brov_ekf_update_from_solver reads the applied records
 * (ahead of the delay stage's flag).  The one-launch closed loop and the *_ticks kernels know no rotors, so the loops take their
 * launch-per-tick branch; a brov_fleet refuses such a solver.  Stage off (the default, and after brov_rotor_off): every launch is the one of
 * a solver without the stage.  Before any brov_rotor_set_host the configuration is tau = 0 everywhere, no limits, h = 0.
 * Out of scope: slew-rate limits, the plugin's propeller efficiency, a lead compensator, the fleet.
 * Refused with BROV_ERR_ARG and a text in brov_last_error() that starts with the call's name (nothing changes, nothing is waited for): a NULL
 * handle, a negative or non-finite tau, a non-finite h, a NaN limit, cmd_lo[i] > cmd_hi[i], a non-finite state. */
int brov_rotor_coeffs(double tau, double h, double* alpha, double* beta);   /* pure host function, needs no device; tau == 0: (0, 0); BROV_ERR_ARG for tau < 0 or not finite, h not finite or <= 0 */
int brov_rotor_set_host(brov_solver* s, const double* tau /*[B][6]; NULL: 0.2 everywhere, the reference's*/, double h /*<= 0: the options' Ts*/,
                        const double* cmd_lo /*[6]; NULL: -inf*/, const double* cmd_hi /*[6]; NULL: +inf*/,
                        int32_t observer_applied);                    /* switches the stage on, zeroes the state, the statistics and the step count */
int brov_rotor_off(brov_solver* s);
int brov_rotor_enabled(const brov_solver* s);                         /* 0 for NULL */
int brov_rotor_reset(brov_solver* s);                                 /* zeroes the state, the statistics and the step count */
int brov_rotor_set_state_host(brov_solver* s, const double* r /*[B][6], finite*/);
int brov_rotor_get_state_host(brov_solver* s, double* r /*[B][6]*/);
int brov_rotor_last_host(brov_solver* s, double* u0_applied /*[B][4]*/, double* thrust_applied /*[B][6]*/);   /* what the last plant step was given; one may be NULL */
int brov_rotor_get_stats_host(brov_solver* s, double* lag_sq /*[B]*/, int64_t* steps);   /* either may be NULL */
int brov_rotor_get_coeffs_host(brov_solver* s, double* alpha /*[B][6]*/, double* beta /*[B][6]*/, double* h);   /* the uploaded values; any may be NULL, not all */
/* the stage alone: applied [B][6] and state_out [B][6] for the commands commanded [B][6] from state [B][6] (NULL: the stage's own); moves nothing */
int brov_rotor_eval_host(brov_solver* s, const double* commanded, const double* state, double* applied, double* state_out);
int brov_rotor_last_seconds(brov_solver* s, double* seconds);         /* the last shift launch, HIP events */

/* ---- sensor stage between the plant and the controller: noisy, biased, quantised, slow and dropped measurements.  Without it the solve, the
 * observer (brov_ekf_update_from_solver) and the estimator (brov_rls_update_from_ekf) read the plant's true state.  While the stage is on they
 * read the MEASURED state ymeas [B][12] instead; the plant, the logs and the tracker keep the true state x0.  The fresh sample of channel c of
 * instance b at measurement index m (the plant's tick counter, brov_plant_wrench_tick), x the true value:
 *     v = (x + bias[b][c]) + sigma[b][c] * n(b, m, c)                              every operation rounded on its own: no FMA
 *     y = quant[c] > 0 ? rint(v / quant[c]) * quant[c] : v                         rint: ties to even; a NaN passes through
 * n is a counter-based variate built from integers alone (a restatement needs no libm and agrees bit for bit): with
 * H(k) = splitmix64_finalise((seed ^ 0x53454E534F52) + (k + 1) * 0x9E3779B97F4A7C15) and k = (b << 32) | (m << 8) | (c << 2) | j, S = the sum of
 * the twelve 16-bit fields of H at j = 0, 1, 2 and n = (S - 393210) / 65536.  This is an Irwin-Hall(12) variate, not a Gaussian: variance
 * 1 - 2^-32, bounded by +-6, kurtosis 2.9 instead of 3.  The dropout draw of (b, m) is u = (H(k) >> 11) * 2^-53 at the channel slot c = 12,
 * j = 0; the fix is dropped iff dropout[b] > 0 && u < dropout[b].  sigma, bias [B][12] and dropout [B] are per instance; quant [12] (0: none),
 * period [12] and the seed are shared by the batch.  Indices are limited to 0 <= m < 2^24.
 * Two kinds of refresh of ymeas (sensor_measure_kernel):
 *   regular, at index m   a dropped fix samples nothing; otherwise channel c takes its fresh sample iff m % period[c] == 0 and else keeps its
 *                         value.  Then the statistics: dropped[b] += drop, err_sq[b][c] += (ymeas[c] - x[c])^2 AFTER the refresh, so a held,
 *                         stale value counts as the error the controller really sees; the host counts the refreshes.
 *   forced, at index m    every channel takes its fresh sample; no dropout draw, the statistics untouched.
 * Regular: behind the plant kernel of brov_plant_step and of every tick of the loops built on it (brov_closed_loop / _ex / _dob / _track), on
 * the same stream, at the counter's new value.  Forced, at the current index: brov_sensor_set_host (which first resets the statistics),
 * brov_set_x0_host / brov_set_x0_device while the stage is on (on their stream), and brov_sensor_measure for a caller that wrote x0 some
 * other way.  A brov_tick_host that brings its own x0 is solved at that x0: the caller supplied the measurement.  The one-launch closed loop
 * and the *_ticks kernels know no sensor: the loops take their launch-per-tick branch.  A loop that would pass index 2^24 is refused before
 * anything is launched.  Out of scope and refused while the stage is on: brov_fleet_step, brov_closed_loop_fleet, brov_closed_loop_fleet_dob.
 * Stage off (the default, and after brov_sensor_off): no extra launch, everything reads x0 as before; the statistics stay readable.
 * Refused with BROV_ERR_ARG and a text in brov_last_error() that starts with the call's name (nothing changes, nothing is waited for): a NULL
 * handle, a NaN or negative sigma or quant, a non-finite bias, period < 1, dropout outside [0, 1], an index outside [0, 2^24). */
int brov_sensor_set_host(brov_solver* s, uint64_t seed, const double* sigma /*[B][12]; NULL: 0*/, const double* bias /*[B][12]; NULL: 0*/,
                         const double* quant /*[12]; NULL: none*/, const int32_t* period /*[12]; NULL: 1*/, const double* dropout /*[B]; NULL: 0*/);
int brov_sensor_off(brov_solver* s);
int brov_sensor_enabled(const brov_solver* s);                 /* 0 for NULL */
int brov_sensor_measure(brov_solver* s, void* stream);         /* forced refresh at the current index */
/* the stage alone: fresh samples of the states x at `index` and the dropout verdicts; moves nothing, touches no statistic (before any
 * brov_sensor_set_host: the defaults) */
int brov_sensor_eval_host(brov_solver* s, int64_t index, const double* x /*[B][12]*/, double* y /*[B][12]*/, int32_t* dropped /*[B] or NULL*/);
int brov_sensor_get_measurement_host(brov_solver* s, double* y /*[B][12]*/);   /* as the last refresh left it (zeros before the first) */
int brov_sensor_get_stats_host(brov_solver* s, int32_t* dropped /*[B]*/, double* err_sq /*[B][12]*/, int64_t* refreshes /*any NULL*/);
int brov_sensor_reset_stats(brov_solver* s);
int brov_sensor_last_seconds(brov_solver* s, double* seconds); /* the measure kernel's last launch, HIP events */

/* ---- ocean current on the plant: moving water, the constant_current block of the reference's simulated world
 * (bluerov2_environ/worlds/ocean_waves.world, underwater_current_plugin; Gauss-Markov arguments in bluerov2_dobmpc/launch/
 * start_dobmpc_demo.launch).  A current is a WORLD-frame water velocity vc = (vx, vy, vz) in m/s, held over a plant tick.  It is not a wrench:
 * at every RK stage it is projected with that stage's attitude, c = R^T vc, and the linear and quadratic damping of the three linear
 * velocity rows are evaluated at the velocity through the water v - c.  Nothing else changes: the state stays the velocity over ground; the
 * controller, the sensor stage, the tracker and the logs see what they saw.  Quasi-static drag only (no added-mass term of a changing current).
 *   BROV_CURRENT_OFF           (default) every launch is the one of a solver without the stage
 *   BROV_CURRENT_CONSTANT      v[B][3]
 *   BROV_CURRENT_TABLE         [rows][3] shared by the batch, row min(k, rows - 1) at plant tick k (the counter brov_plant_wrench_tick reads),
 *                              times gain[b]: one rounded product
 *   BROV_CURRENT_GAUSS_MARKOV  the plugin's first-order process per WORLD AXIS (not in speed and two angles), with DEVICE state c[B][3].  A plant
 *                              step at counter tick k integrates under c as it stands and then advances it, for axis i of instance b:
 *                                  U  = (splitmix64_finalise(seed + (n + 1) * 0x9E3779B97F4A7C15) >> 11) * 2^-53,  n = (b << 24) | (k << 2) | i
 *                                  xi = 2 U - 1
 *                                  v  = (c[i] - step * (mu[i] * (c[i] - mean[b][i]))) + amp[i] * xi        every operation rounded on its own
 *                                  c[i] = v < lo[i] ? lo[i] : (v > hi[i] ? hi[i] : v)
 *                              (the periodic wrench's counter draw with the tick in place of the half period; channel 3 stays reserved).
 *                              Entering the mode sets c = mean.  The tick field has 22 bits: a step or loop that would draw at a tick >= 2^22
 *                              is refused before anything is launched.  brov_plant_wrench_seek moves the noise counter only; the state is
 *                              set with brov_current_set_state_host.  One lane per instance, no atomics: bit-reproducible.
 * With a mode in force brov_plant_step and every loop built on it (brov_closed_loop / _ex / _dob / _track) launch plant_current_kernel, behind
 * the thruster stage and under the wrench mode in force, with their statistics and logs as ever; the one-launch closed loop knows no current,
 * so the loops take their launch-per-tick branch.  This current is indexed by the INSTANCE: brov_fleet_step, brov_closed_loop_fleet and
 * brov_closed_loop_fleet_dob refuse a solver with a mode in force; the water a fleet's vehicles move in is set with brov_vehicle_current_*.
 * Refused with BROV_ERR_ARG and a text in brov_last_error() that starts with the call's name (nothing changes, nothing is waited for): a NULL
 * handle or array, a non-finite value, lo[i] > hi[i], step < 0, rows < 1, a negative tick. */
#define BROV_CURRENT_OFF 0
#define BROV_CURRENT_CONSTANT 1
#define BROV_CURRENT_TABLE 2
#define BROV_CURRENT_GAUSS_MARKOV 3
int brov_current_constant_host(brov_solver* s, const double* v /*[B][3]*/);
int brov_current_table_host(brov_solver* s, const double* tab /*[rows][3]*/, int rows, const double* gain /*[B] or NULL*/);
int brov_current_gauss_markov_host(brov_solver* s, uint64_t seed, const double* mean /*[B][3]*/, const double* mu /*[3]*/, const double* amp /*[3]*/,
                                   const double* lo /*[3]; NULL: -5*/, const double* hi /*[3]; NULL: 5*/, double step /*seconds per tick*/);
int brov_current_off(brov_solver* s);
int brov_current_mode(const brov_solver* s);                                   /* BROV_CURRENT_*; OFF for NULL */
/* the current of every instance at `tick` in CONSTANT / TABLE mode (zeros while OFF); moves nothing; refused in GAUSS_MARKOV mode */
int brov_current_eval_host(brov_solver* s, int64_t tick, double* v /*[B][3]*/);
int brov_current_get_state_host(brov_solver* s, double* v /*[B][3]*/);         /* what the next plant step applies */
int brov_current_set_state_host(brov_solver* s, const double* v /*[B][3]*/);   /* GAUSS_MARKOV only */
int brov_current_last_host(brov_solver* s, double* v /*[B][3]*/);              /* of the last plant step under a current (zeros before the first) */
int brov_current_last_seconds(brov_solver* s, double* seconds);                /* plant_current_kernel's last launch, HIP events */

/* ---- Coriolis and centripetal forces on the plant: the vehicle the reference's observer is written for.  The OCP model, which the plant
 * integrates, drops the Coriolis products of the linear axes; BLUEROV2_DOB::f() (bluerov2_dob.cpp:651-677) has the rigid-body ones, and the
 * reference's simulated world is a Fossen model with C_RB + C_A (dynamics_C(), :894-906).  With the stage on, the plant adds rows X, Y, Z, N of
 * -C_RB(nu) nu and / or -C_A(nu_r) nu_r for a diagonal added mass and the CG at the origin.  At an RK stage point with body velocities
 * (u, v, w, p, q, r), the velocity through the water (ur, vr, wr) (= (u, v, w) without a current), m = 11.26 and the instance's TRUE plant
 * parameters Xa, Ya, Za = p[4..6]:
 *   BROV_CORIOLIS_RIGID   cX = m ((r v) - (q w))     cY = m ((p w) - (r u))     cZ = m ((q u) - (p v))     cN = 0
 *   BROV_CORIOLIS_ADDED   ax = Xa ur, ay = Ya vr, az = Za wr;  bx = ka p, by = ma q
 *                         aX = (ay r) - (az q)       aY = (az p) - (ax r)       aZ = (ax q) - (ay p)
 *                         aN = ((ax vr) - (ay ur)) + ((bx q) - (by p))
 *   both (3)              one add per channel, rigid + added
 * every product and every difference rounded on its own, in the order written.  The forces enter where the model's own disturbances do (dx, dy,
 * dz, dn, ahead of the mass scaling) and are evaluated afresh at every RK stage.  The RIGID group is exactly what the EKF's f() has.  Nothing
 * else changes: the inertias stay the model's; the controller, the delay stage's predictor, the EKF and the RLS keep their models.  The roll and
 * pitch rows of C_A are deliberately left out.  ka, ma: the roll / pitch added inertia (the reference: 0 and 1.2481).
 * With the stage on brov_plant_step and every loop built on it (brov_closed_loop / _ex / _dob / _track) launch plant_coriolis_kernel, behind
 * the delay, rotor and thruster stages, under the wrench mode and in the current in force, with their statistics and logs as ever; the
 * one-launch closed loop does not know the stage, so the loops take their launch-per-tick branch.  Off (default): every launch is the one of a
 * solver without the stage.  This stage is indexed by the INSTANCE: brov_fleet_step, brov_closed_loop_fleet and brov_closed_loop_fleet_dob
 * refuse a solver with the stage on; the stage of a fleet's vehicles is set with brov_vehicle_coriolis_*.
 * Refused with BROV_ERR_ARG and a text in brov_last_error() that starts with the call's name (nothing changes, nothing is waited for): a NULL
 * handle or array, terms outside 1 ... 3, ka or ma non-finite or negative. */
#define BROV_CORIOLIS_RIGID 1
#define BROV_CORIOLIS_ADDED 2
int brov_coriolis_set(brov_solver* s, int terms /*1..3*/, double ka, double ma);
int brov_coriolis_off(brov_solver* s);
int brov_coriolis_terms(const brov_solver* s);                                 /* the bit mask in force; 0 for NULL or off */
int brov_coriolis_get(const brov_solver* s, int* terms, double* ka, double* ma);   /* as last set (terms 0 while off; before any set: 0, 0, 1.2481) */
/* the force alone, c = [X Y Z N] per instance, at the states x in water moving with the world-frame velocities vc (NULL: still water), with
 * the terms in force (off: zeros) and the plant parameters the next plant step would use.  vc is projected with the state's attitude as the
 * model does, every operation rounded on its own.  Moves nothing */
int brov_coriolis_eval_host(brov_solver* s, const double* x /*[B][12]*/, const double* vc /*[B][3] or NULL*/, double* c /*[B][4]*/);
int brov_coriolis_last_host(brov_solver* s, double* c /*[B][4]*/);            /* at the start state of the last plant step under the stage (zeros before the first) */
int brov_coriolis_last_seconds(brov_solver* s, double* seconds);               /* plant_coriolis_kernel's last launch, HIP events */

/* iterate (warm start) access; any pointer may be NULL to skip that block */
int brov_set_iterate_host(brov_solver* s, const double* x, const double* u, const double* pi, const double* lam);
int brov_get_iterate_host(brov_solver* s, double* x, double* u, double* pi, double* lam);
int brov_reset(brov_solver* s); /* zero iterate like bluerov2_acados_reset */
int brov_init_iterate_default(brov_solver* s); /* create-time default iterate */

/* one RTI step for all B instances, enqueued on `stream` (NULL = default).  Asynchronous: returns after launch. */
int brov_solve(brov_solver* s, void* stream);
/* acados' rti_phase (main_bluerov2.c:217): 0 = preparation + feedback (== brov_solve), 1 = preparation only
 * (linearise at the current iterate), 2 = feedback only (QP + step with the current x0; needs a prior phase 1).  Batches of at most one
 * instance per CU at N <= 81: the preparation also runs the step-0 factor sweep -- it does not depend on x0 -- and
 * parks the factorised LDS image; the feedback is forward sweep + bound check + step + record (a batch of one at N = 80 through
 * brov_tick_host: 33 us from the measurement to u0, against 71 us for rti_phase 0); a call that changes the iterate, the grid or the options
 * between the two makes the feedback fail (BROV_ERR_ARG: repeat the preparation) -- and so does a feedback call with no fresh preparation
 * at all (none since the last step, e.g. a second rti_phase 2 on one preparation): the iterate that was linearised is gone.  acados itself
 * would re-solve the QP in its memory; the acados-shaped drop-in turns such a call into a whole step (rti_phase 0) instead of failing.
 * Elsewhere: linearisation / QP on the streaming pair. */
int brov_solve_phase(brov_solver* s, void* stream, int rti_phase);
/* `ticks` consecutive RTI steps of every instance, the measured state held, the shared reference window moving on `row_stride` rows of the
 * resident trajectory table per step (0: the window in force stays -- several SQP iterations on one problem, e.g. candidates iterated to
 * convergence; > 0 needs the window to come from brov_set_yref_from_traj).  Result: exactly that of
 *     for k in 0 .. ticks-1: brov_set_yref_from_traj(s, line + k * row_stride, ncols, stream); brov_solve(s, stream)
 * (records of the last step; status_log, DEVICE [ticks][B] or NULL, keeps every step's status) -- but on the uniform grid it is ONE launch in
 * which every instance goes on to its next step as soon as its own is done (rti_fused_kernel_ticks for N <= 23, rti_window_kernel_ticks for
 * longer horizons and batches beyond two instances per CU; smaller batches at long horizons, general grids and the streaming pair take a
 * launch per step): a step with a slow instance -- 13 .. 47 Newton systems on a diverging one -- no longer holds the whole batch at a
 * launch boundary, and there are no launch gaps.  For workloads whose steps do not depend on each other through the host (parameter sweeps,
 * candidate libraries, Monte-Carlo draws at a fixed measurement); a control loop that measures between two steps calls brov_solve. */
int brov_solve_ticks(brov_solver* s, void* stream, int ticks, int row_stride, int32_t* status_log /*DEVICE or NULL*/);
int brov_synchronize(brov_solver* s, void* stream);
/* Stream ordering.  One solver, one stream at a time: every call that enqueues work (brov_solve*, brov_plant_step, the *_device
 * setters, the trajectory / candidate window builders, brov_ekf_*_solver) first waits -- on the host -- for the stream the solver
 * used LAST when that is a different one (e.g. brov_tick_host's private stream, whose kernel may still be finishing when the tick
 * returns its records).  Calls on the same stream cost nothing.  brov_order_stream does the same wait explicitly, for callers that
 * work on the DEVICE pointers handed out below from a stream of their own. */
int brov_order_stream(brov_solver* s, void* stream);
/* One control tick with ONE host synchronisation: the inputs that changed since the last tick (NULL = unchanged; x0 [B][12], ONE
 * reference window shared by the batch [N+1][16], per-stage parameters [B][N+1][16]) are staged through a pinned buffer and copied
 * asynchronously on the solver's own stream, the step (rti_phase as brov_solve_phase) runs behind them, the result records come
 * back the same way -- for up to 64 instances without a copy: the kernel writes each record into the pinned buffer itself, followed
 * by a sequence word the host polls (BROV_TICK_MAILBOX=0 in the environment at brov_create: copy + stream synchronisation, as for larger
 * batches).  A tick that passes all three inputs uploads them with one copy.  This is what the acados-shaped drop-in makes of one
 * bluerov2_acados_solve (bluerov2_dob.cpp:306-388: lbx / ubx, (N+1) x update_params, (N+1) x yref, solve, u0 / status / kkt).
 * rti_phase 1 (a preparation) delivers no records: the call returns as soon as the inputs have left the pinned buffer, `res` is left alone,
 * and the preparation runs on, stream-ordered ahead of whatever follows.  HOST pointers. */
int brov_tick_host(brov_solver* s, const double* x0, const double* yref_shared, const double* par_stage, int rti_phase,
                   brov_result* res /*[B] or NULL*/);
/* The staging buffers brov_tick_host copies its arguments into / its records out of: device-visible pinned host memory, valid until
 * brov_destroy.  A caller that builds its inputs in them and reads its records from them -- pass exactly these pointers as x0 /
 * yref_shared / par_stage, and NULL as res -- saves the tick its host-side copies (0.8 MB per step at a batch of 4096).  The result
 * records are written there by the solve kernel itself (no copy command behind the launch; batches <= 64: with a sequence word per
 * instance that the host polls, larger ones: the host waits for the launch once; BROV_TICK_BULK=0: the copy command of round 3).
 * The input buffers may be rewritten as soon as brov_tick_host has returned (a tick that was handed these pointers waits for the copies it
 * enqueued out of them; a tick that copies its arguments in waits, before it does, for what an earlier tick left reading them). */
/* instrumentation: which instances of the last solve were completed by the parallel-in-time kernel */
int brov_pit_last(brov_solver* s, int32_t* done /*[B]*/);
int brov_tick_buffers(brov_solver* s, double** x0 /*[B][12]*/, double** yref_shared /*[N+1][16]*/, double** par_stage /*[B][N+1][16]*/,
                      const brov_result** res /*[B]*/);
/* Development knobs.  The solver's A/B switches and test hooks are BROV_* environment variables (BROV_PIT, BROV_TICK_MAILBOX,
 * BROV_PARTIAL_REFACTOR, ...: DESIGN.md section 4.6 lists them); a solver reads them ONCE, in brov_create -- no call on the path of a
 * solve touches the environment.  brov_dev_reload_knobs reads them again (tests that flip a switch between two solves of one solver). */
int brov_dev_reload_knobs(brov_solver* s);
/* BROV_TICK_BREAKDOWN=1: host microseconds of the last brov_tick_host -- staging, launch, post-launch enqueues, wait for the records, total */
int brov_dev_tick_breakdown(brov_solver* s, double us[5]);
/* replace weights / bounds / Ts / QP options of an existing solver (N must not change) */
int brov_set_opts(brov_solver* s, const brov_opts* opts);
int brov_get_opts(const brov_solver* s, brov_opts* opts);

/* outputs */
int brov_get_results_host(brov_solver* s, brov_result* res /*[B]*/); /* syncs the last solve's stream */
int brov_get_u0_host(brov_solver* s, double* u0 /*[B][4]*/);
const brov_result* brov_results_device(const brov_solver* s);          /* DEVICE pointer, [B] records */
/* DEVICE pointers to the resident state for zero-copy producers/consumers (layouts above) */
double* brov_x0_device(brov_solver* s);
double* brov_yref_device(brov_solver* s);   /* [B][N+1][16] (always allocated; used when shared == 0) */
double* brov_params_device(brov_solver* s); /* [B][N+1][16] */
double* brov_x_device(brov_solver* s);
double* brov_u_device(brov_solver* s);
/* linearisation of the LAST solve (row-major per stage: [A|B] as [12][16], b as [12]).  The streaming path always leaves it
 * in HBM; the LDS-resident kernels write it out only after brov_debug_dump_linearisation(s, 1).  For tests. */
int brov_get_linearisation_host(brov_solver* s, double* AB /*[B][N][12][16]*/, double* b /*[B][N][12]*/);
int brov_debug_dump_linearisation(brov_solver* s, int enable);

/* ---- boundary corners of the reference API -----------------------------------------------------------------------------------
 * Non-uniform grids: bluerov2_acados_create_with_discretization(capsule, N, new_time_steps) / bluerov2_acados_update_time_steps
 * (c_generated_code/acados_solver_bluerov2.h:141,146; .c:111-131) set the ERK4 step AND the cost scaling of stage i to
 * new_time_steps[i].  brov_set_time_steps does the same for the whole batch (ts[N]; NULL or a uniform vector = the uniform grid
 * with brov_opts::Ts).  Separate stage-0 weight: the generated solver carries W_0 next to W (.c:422-441, same numbers as
 * shipped); brov_set_stage0_weight(W0[16]) gives stage 0 its own (NULL or W itself = one stage weight).
 * Round 4: either feature runs on the LDS-resident kernels (grid instantiations of the fused kernel, of the windowed kernel, of its
 * resident mode and of the parallel-in-time step-0 kernel of small batches) as well as on the streaming pair. */
int brov_set_time_steps(brov_solver* s, const double* ts /*[N] or NULL*/);
int brov_set_stage0_weight(brov_solver* s, const double* W0 /*[16] or NULL*/);
int brov_general_grid(const brov_solver* s);   /* 1 while either feature is in force */

/* ---- 6-disturbance model variant (BASELINE configs[2] "6 disturbance states") ------------------
 * The reference's EKF estimates six disturbances (bluerov2_dob.h:200-205), its OCP model takes four: the roll / pitch symbols are
 * there but commented out (bluerov2_dobmpc/scripts/bluerov2.py:37-38), so the shipped solver has np = 16.  This switch (default
 * OFF = the shipped model) adds the two terms the way the other four enter their rows (bluerov2.py:123-128):
 *     dp += d_phi / Ix,   dq += d_theta / Iy            (additive: df/dx and df/du are untouched)
 * with d_phi, d_theta per instance and stage, next to p[16].  brov_set_params18_host takes the parameter vector the uncommented
 * model would have, [dx dy dz d_phi d_theta d_psi | added mass 4 | linear damping 4 | quadratic damping 4]; with the variant on,
 * brov_ekf_apply_to_solver fills all six disturbances from the estimate, and brov_plant_step integrates the controller's stage-0
 * values unless brov_plant_set_rp_disturbance_host gave the plant its own. */
int brov_enable_dist6(brov_solver* s, int on);
int brov_dist6_enabled(const brov_solver* s);
int brov_set_rp_disturbance_host(brov_solver* s, const double* d /*[B][2] or [B][N+1][2]*/, int per_stage);
int brov_set_rp_disturbance_device(brov_solver* s, const double* d, int per_stage, void* stream);
int brov_set_params18_host(brov_solver* s, const double* p18 /*[B][18] or [B][N+1][18]*/, int per_stage);
double* brov_rp_disturbance_device(brov_solver* s);   /* [B][N+1][2]; NULL while the variant is off */
int brov_get_rp_disturbance_host(brov_solver* s, double* d /*[B][N+1][2]*/);
int brov_plant_set_rp_disturbance_host(brov_solver* s, const double* d /*[B][2]; NULL: back to the controller's stage 0*/);

/* argmin of cost over the eligible instances -- status SUCCESS and a finite cost: NaN, +Inf and -Inf never win; ties: lowest index; the
 * one rule of bluerov2_amd/csrc/select_device.hpp -- (config 4 "best-trajectory select"); writes the winning index (-1: no instance
 * qualifies) and its record; runs on the GPU, result copied to HOST */
int brov_select_best_host(brov_solver* s, int* best_index, brov_result* best);

/* ---- several GPUs in ONE process (BASELINE.json configs[3]: 65 536 candidates over 8 GPUs, all-gather of the
 * optimal cost / u* for best-trajectory select) ------------------------------------------------------------------------------------
 * A group owns one brov_solver per device -- a contiguous shard of `total_instances`, the first total % n shards one instance
 * larger --, one stream and one RCCL communicator per device.  There is no communication during the solve; brov_group_gather is ONE
 * ncclAllGather per device (inside ncclGroupStart / ncclGroupEnd, on the devices' own streams, behind the solve) of
 *     BROV_GATHER_RECORDS  every instance's 104-byte result record, to every device (uneven shards: padded with never-selectable slots)
 *     BROV_GATHER_PACKED   one (cost, global index) pair per device (16 B): the local arg-min -- when only the winner is wanted
 * and brov_group_select_best returns the global arg-min of cost over the instances with status SUCCESS and a finite cost (NaN, +Inf and
 * -Inf never win; ties: lowest index; the rule of bluerov2_amd/csrc/select_device.hpp, as brov_select_best_host) and waits
 * for it -- the only host wait of a step.  With BROV_GATHER_RECORDS the winner comes back through a pinned host mailbox the select kernel
 * (up to 64 blocks over the gathered records) writes itself: no copy command and no stream synchronisation on the way back; the call
 * returns when local device 0 has delivered, the other devices may still be finishing their gather (their streams order whatever is
 * enqueued next behind it; brov_group_synchronize waits for all of them).  Per-shard inputs go through the shard's own handle (brov_group_solver: every brov_set_* /
 * brov_get_* above works on it, with brov_group_stream(rank) as the stream) or through the whole-batch setters below, which slice a
 * global HOST array.  RCCL is loaded at run time (dlopen) by brov_group_create; a process that never creates a group never loads it.
 * The reference's callers live in one C++ process (bluerov2_dob.cpp:270-451): this is their route to several GPUs; one process per
 * GPU on torch.distributed (bluerov2_amd/distributed.py, bench.py --gpus N) is the other. */
typedef struct brov_group brov_group;
#define BROV_GATHER_RECORDS 0
#define BROV_GATHER_PACKED 1
int  brov_group_create(brov_group** out, const int* devices /*[n] distinct HIP ordinals*/, int n, int total_instances, const brov_opts* opts);
/* Which collective carries the gather.  BROV_COLLECTIVE_RCCL (what brov_group_create / brov_group_create_rank use): ncclAllGather.
 * BROV_COLLECTIVE_COPY: the all-gather as device-to-device copies -- every rank publishes its contribution behind an event on its own
 * stream, every rank pulls the others' into its own gathered array on its own stream.  RCCL is not loaded, and `devices` may name a GPU
 * more than once: W ranks on ONE GPU run the whole bookkeeping of W GPUs (shard bounds, padded staging, rank-major gathered layout, packed
 * pairs, the select over W x slots) -- the development and test route on a 1-GPU box, and a fallback where RCCL is not installed.  The
 * ranks of a copy group live in ONE process; brov_group_gather blocks the calling thread until every rank of the group has entered the
 * same gather (ranks held by other brov_group objects: call from one thread per object, as RCCL asks of ncclCommInitRank ranks that share
 * a process), and the id of brov_group_create_rank_ex may be any 128 bytes the ranks agree on.  The entry points put the calling thread's
 * current HIP device back before they return. */
#define BROV_COLLECTIVE_RCCL 0
#define BROV_COLLECTIVE_COPY 1
int  brov_group_create_ex(brov_group** out, const int* devices /*[n]*/, int n, int total_instances, const brov_opts* opts, int collective);
/* The same group with ONE PROCESS PER GPU (the launcher's route, e.g. torchrun): every process creates its rank of the group on its own
 * device.  Rank 0 calls brov_group_unique_id and hands the 128 bytes to the other ranks by whatever means the launcher has (a file, MPI,
 * torch.distributed.broadcast); counts[world] = instances per rank.  All entry points below then act on the local shard, the gather
 * spans all ranks; brov_group_select_best returns the global index everywhere and the full record where the winner is local or the
 * 104-byte records were gathered (with BROV_GATHER_PACKED and a remote winner: cost and status only). */
int  brov_group_unique_id(char id[128]);
int  brov_group_create_rank(brov_group** out, int device, int rank, int world, const char id[128], const int* counts /*[world]*/, const brov_opts* opts);
int  brov_group_create_rank_ex(brov_group** out, int device, int rank, int world, const char id[128], const int* counts /*[world]*/, const brov_opts* opts,
                               int collective);
int  brov_group_collective(const brov_group* g);     /* BROV_COLLECTIVE_* */
int  brov_group_set_copy_wait_seconds(int seconds);  /* BROV_COLLECTIVE_COPY: how long a gather waits for a rank that has not entered it (60) */
void brov_group_destroy(brov_group* g);
const char* brov_group_last_error(void);
int  brov_group_rccl_version(int* version);          /* loads RCCL if need be; BROV_ERR_HIP when it cannot be loaded */
int  brov_group_size(const brov_group* g);           /* devices held by THIS process (local indices 0 .. size-1 address solver / stream below) */
int  brov_group_world(const brov_group* g);          /* ranks of the whole group (= size in the one-process form) */
int  brov_group_first_rank(const brov_group* g);     /* global rank of local device 0 */
int  brov_group_total(const brov_group* g);
int  brov_group_shard(const brov_group* g, int rank, int* lo, int* hi);   /* global instance range [lo, hi) of GLOBAL rank `rank` */
brov_solver* brov_group_solver(brov_group* g, int local);   /* shard handle of local device `local` */
void* brov_group_stream(brov_group* g, int local);    /* its hipStream_t */
int brov_group_set_x0_host(brov_group* g, const double* x0 /*[total][12]*/);
int brov_group_set_params_host(brov_group* g, const double* p /*[total][16] or [total][N+1][16]*/, int per_stage);
int brov_group_set_yref_host(brov_group* g, const double* yref /*shared [N+1][16] or [total][N+1][16]*/, int shared);
int brov_group_set_candidate_params_host(brov_group* g, int kind, const double* p0, const double* p1, const double* phase /*[total]*/);
int brov_group_set_yref_candidates(brov_group* g, double t0, double dt);   /* one window kernel per device, no host traffic */
int brov_group_solve(brov_group* g);                 /* one RTI step of every shard, enqueued; returns after the launches */
int brov_group_gather(brov_group* g, int mode);      /* enqueued behind the solve */
int brov_group_select_best(brov_group* g, int* best_index /*global; -1: no instance qualifies*/, brov_result* best /*or NULL*/);
int brov_group_synchronize(brov_group* g);
int brov_group_get_results_host(brov_group* g, brov_result* res /*[total]*/);   /* after a BROV_GATHER_RECORDS gather: device 0's copy */
const brov_result* brov_group_gathered_device(const brov_group* g, int rank);   /* DEVICE: [n][slots_per_rank] records on shard `rank`'s GPU */
int brov_group_slots_per_rank(const brov_group* g);
int brov_group_enable_timing(brov_group* g, int on);  /* HIP events around solve / gather / select (default on) */
int brov_group_last_seconds(brov_group* g, double* solve, double* gather, double* select);   /* slowest device each */

/* thrust allocation (bluerov2_dob.cpp:390-395): t[B][6] = the `thrust` field the solve kernel wrote into every result record */
int brov_get_thrusts_host(brov_solver* s, double* t6 /*[B][6]*/);

/* timing of the last brov_solve (HIP events on its stream), seconds: total and per kernel [linearise, qp] */
int brov_last_solve_seconds(brov_solver* s, double* total, double* kernels2);
int brov_enable_timing(brov_solver* s, int on);
/* which kernels the last brov_solve launched: BROV_PATH_FUSED, BROV_PATH_WINDOWED or BROV_PATH_STREAMING */
int brov_last_kernel_path(const brov_solver* s);
/* stages per LDS window of the windowed kernel this solver was created for (0: no windowed workspace).  Equal to N: resident mode,
 * the whole horizon in one window (batches of at most one instance per CU at N <= 81); otherwise <= 20 */
int brov_window_stages(const brov_solver* s);
/* what the LDS-resident kernel this solver launches asks of a compute unit: info = {dynamic LDS bytes per block (= per instance in
 * flight), blocks per CU granted by the occupancy query, threads per block, kind: 1 whole horizon / 2 whole horizon, two waves per
 * SIMD / 3 windowed / 4 windowed, resident mode}; all 0 when the solver runs on the streaming kernels */
int brov_lds_kernel_info(const brov_solver* s, int32_t info[4]);

/* ---------------------------------------------------------------------------------------------------------------------
 * Batched EKF disturbance observer: B independent copies of the reference's 18-state filter
 * BLUEROV2_DOB::EKF() (bluerov2_dobmpc/src/bluerov2_dob.cpp:495-545) -- forward-difference Jacobians of the RK4 map
 * (:730-744, with the k2/3 stage quirk of :630) and of the measurement model (:747-762), gain through the explicit
 * inverse of the innovation covariance, Joseph-form covariance update.  One call = one EKF tick of every instance.
 * State [pose(6) | body velocities(6) | body-frame disturbance wrench(6)], instance-major, FP64.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct brov_ekf brov_ekf;
typedef struct brov_ekf_params { /* defaults: bluerov2_dob.h:171-183,208 and bluerov2_dob.cpp:41-62 */
    double dt;
    double mass, Ix, Iy, Iz, ZG, g, bouyancy;
    double added_mass[6], Dl[6], Dnl[6];
    double K[36];          /* propulsion matrix, row-major: tau = K * thrust */
    double Q[18];          /* process noise (diagonal) */
    double R;              /* measurement noise R * I */
    double fd_step;        /* finite-difference step of both Jacobians (1e-6) */
    double compensate_coef, rotor_constant; /* scaling of the estimate into the NMPC parameters p[0..3] (:334-337) */
} brov_ekf_params;
void brov_ekf_default_params(brov_ekf_params* p);
const char* brov_ekf_last_error(void); /* message of the last failing brov_ekf_* call on this thread */
int  brov_ekf_create(brov_ekf** out, int device, int batch, const brov_ekf_params* p /* NULL: defaults */);
void brov_ekf_destroy(brov_ekf* e);
int  brov_ekf_batch(const brov_ekf* e);
/* every instance := (x0, P0); NULL = the reference's start [0,0,-20,0..0,6,6,6,0,0,0], P0 = I (bluerov2_dob.cpp:64-65) */
int brov_ekf_reset(brov_ekf* e, const double* x0 /*[18]*/, const double* P0 /*[18][18]*/);
int brov_ekf_set_state_host(brov_ekf* e, const double* x /*[B][18]*/, const double* P /*[B][18][18]*/);
int brov_ekf_get_state_host(brov_ekf* e, double* x /*[B][18] or NULL*/, double* P /*[B][18][18] or NULL*/);
/* one EKF tick.  thrust = meas_u (thruster outputs, :498), y12 = measured pose + body velocities (:501-502), acc = body
 * accelerations (finite differences of the velocities, :148-153).  HOST or DEVICE pointers respectively. */
int brov_ekf_update_host(brov_ekf* e, const double* thrust /*[B][6]*/, const double* y12 /*[B][12]*/,
                         const double* acc /*[B][6]*/, void* stream);
int brov_ekf_update_device(brov_ekf* e, const double* thrust, const double* y12, const double* acc, void* stream);
/* outputs of the last tick: world-frame disturbance (:540-545), NMPC parameters p[0..3] (:334-337), per-instance status
 * (0 ok; 1 innovation covariance not positive definite or NaN: estimate and covariance left at the prediction x_pred,
 *  F P F' + Q -- the covariance exactly symmetric -- and wf, mpc_p made from that estimate;
 *  2 non-finite estimate, e.g. a NaN measurement: propagated as the reference would) */
int brov_ekf_get_outputs_host(brov_ekf* e, double* wf /*[B][6] or NULL*/, double* mpc_p /*[B][4] or NULL*/,
                              int* status /*[B] or NULL*/);
const double* brov_ekf_x_device(const brov_ekf* e);      /* [B][18] */
const double* brov_ekf_P_device(const brov_ekf* e);      /* [B][18][18] */
const double* brov_ekf_mpc_p_device(const brov_ekf* e);  /* [B][4] */
/* close the DOB-MPC loop on the device (BASELINE config 3), no host round trip:
 *   brov_ekf_update_from_solver: measurement = the solver's x0 (the plant state after brov_plant_step), thrusts = thrust
 *     allocation of the solver's last u0 (:390-395) -- the thruster vector brov_plant_step applies --, accelerations =
 *     (v - v_prev)/dt with v_prev kept in the observer (zero after brov_ekf_reset, like the reference's pre_body_pos);
 *   brov_ekf_apply_to_solver: p[0..3] of every stage of instance b := the estimate of instance b (:332-337).
 * Units: the reference's plant is Gazebo, whose thrusters turn a command w into rotor_constant*w|w| newtons, and :334-337
 * rescale the estimated wrench by 1/compensate_coef resp. 1/rotor_constant into the OCP model's force units.  The device
 * plant is the OCP model itself (wrench = K * allocation(u)/rotor_constant), so an observer that is to compensate THAT
 * plant is created with compensate_coef = rotor_constant = 1 in brov_ekf_params. */
int brov_ekf_update_from_solver(brov_ekf* e, brov_solver* s, void* stream);
int brov_ekf_apply_to_solver(brov_ekf* e, brov_solver* s, void* stream);
/* seconds of the last update kernel (HIP events on its stream) */
int brov_ekf_last_update_seconds(brov_ekf* e, double* seconds);

/* ---------------------------------------------------------------------------------------------------------------------
 * Batched RLS-FF parameter estimator of the adaptive MPC node: B independent copies of the reference's recursive least squares
 * with a variable forgetting factor BLUEROV2_AMPC::RLSFF() (bluerov2_dobmpc/src/bluerov2_ampc.cpp:731-1046), which the node runs
 * every tick between the EKF and the solve (bluerov2_ampc_node.cpp:28-30).  Four independent axes a = X, Y, Z, N (surge, sway,
 * heave, yaw; the reference's K / M axes are never updated), each with theta in R^4 (0 at start), P in R^4x4 (p0 I), lambda (lambda0)
 * and two windows of prediction errors (n_short = FF_n, n_long = FF_d, bluerov2_ampc.h:239-240).  One tick of axis a:
 *     x = [acc_a, v_a, 1, v_a |v_a|]  (acc = (v - v_prev)/dt of pose_cb, :163-168),  y = the EKF's disturbance estimate esti_x(12|13|14|17)
 *     e = y - x.theta;  e pushed onto both windows;  F = var_short / var_long  (mean = sum / size, var = sum (v - mean)^2 / size)
 *     F > threshold: lambda -= step, not below lambda_min;  else lambda += step, not above lambda_max   (:776-793; the first tick's
 *                    0/0 = NaN is not > threshold)
 *     K = P x / (lambda + x.(P x)),  theta += K e,  P = (P - (K x^T) P) / lambda
 * and the world-frame environmental disturbance wf_env from theta(2) and the measured Euler angles (:1000-1005, rows 4-6 as written
 * there).  theta, P, lambda, F and e are bit-identical to a scalar restatement of these formulas (sums in index order, no FMA
 * contraction, no reciprocals); wf_env goes through sin / cos.  State instance-major on the host side, axis order X, Y, Z, N, FP64.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct brov_rls brov_rls;
typedef struct brov_rls_params { /* defaults: bluerov2_ampc.h:171-180,239-240 and bluerov2_ampc.cpp:735,776-793 */
    int32_t n_short, n_long;       /* window lengths, 5 / 50; each in [1, 256] */
    double  threshold;             /* 0.8 */
    double  lambda_step;           /* 0.01 */
    double  lambda_min, lambda_max;/* 0.5, 1 */
    double  lambda0;               /* 0.9; 0 < lambda_min <= lambda0 <= lambda_max */
    double  p0;                    /* 1: P = p0 I after brov_rls_reset */
    double  dt;                    /* 0.05: the accelerations of brov_rls_update_from_ekf; > 0 */
    double  compensate_coef, rotor_constant;   /* AMPC's scaling of theta(2) into the NMPC parameters p[0..3] (:346-349) */
} brov_rls_params;
#define BROV_RLS_APPLY_DISTURBANCE 0   /* the shipped AMPC: p[0..3] only */
#define BROV_RLS_APPLY_MODEL 1         /* also p[4..15] = theta(0), theta(1), theta(3) of X, Y, Z, N (the commented-out :355-378) */
void brov_rls_default_params(brov_rls_params* p);
const char* brov_rls_last_error(void); /* message of the last failing brov_rls_* call on this thread */
int  brov_rls_create(brov_rls** out, int device, int batch, const brov_rls_params* p /* NULL: defaults */);
void brov_rls_destroy(brov_rls* r);
int  brov_rls_batch(const brov_rls* r);
/* every instance: theta = 0, P = p0 I, lambda = lambda0, both windows empty, v_prev = 0 */
int brov_rls_reset(brov_rls* r);
/* HOST state; NULL skips that block.  set_state empties the windows. */
int brov_rls_set_state_host(brov_rls* r, const double* theta /*[B][4][4]*/, const double* P /*[B][4][4][4]*/, const double* lambda /*[B][4]*/);
int brov_rls_get_state_host(brov_rls* r, double* theta /*[B][4][4]*/, double* P /*[B][4][4][4]*/, double* lambda /*[B][4]*/,
                            double* F /*[B][4], last tick*/, double* e /*[B][4], last tick*/);
/* one RLS-FF tick of every instance and axis.  y = target (the EKF's body-frame disturbance estimate), acc / vel = body
 * acceleration and velocity (u, v, w, r), rpy = measured Euler angles (wf_env only).  HOST or DEVICE pointers respectively. */
int brov_rls_update_host(brov_rls* r, const double* y /*[B][4]*/, const double* acc /*[B][4]*/, const double* vel /*[B][4]*/,
                         const double* rpy /*[B][3]*/, void* stream);
int brov_rls_update_device(brov_rls* r, const double* y, const double* acc, const double* vel, const double* rpy, void* stream);
/* the on-device AMPC tick (no host round trip): measurement = the solver's x0 (the plant state after brov_plant_step: u, v, w, r and
 * the Euler angles), acc = (v - v_prev)/dt with v_prev kept here, target = the EKF's estimate x[12, 13, 14, 17]; ordered behind the
 * solver's last stream (brov_order_stream) and behind the EKF's last update. */
int brov_rls_update_from_ekf(brov_rls* r, const brov_ekf* ekf, brov_solver* s, void* stream);
/* AMPC's parameter hand-off to every stage of instance b (:346-349): p[0] = theta_X(2)/compensate_coef, p[1] = theta_Y(2)/compensate_coef,
 * p[2] = theta_Z(2)/rotor_constant, p[3] = theta_N(2)/rotor_constant.  BROV_RLS_APPLY_DISTURBANCE leaves p[4..15] and the 6-disturbance
 * variant's roll / pitch values alone; BROV_RLS_APPLY_MODEL also writes p[4+a] = theta_a(0), p[8+a] = theta_a(1), p[12+a] = theta_a(3).
 * (The reference with COMPENSATE_D == false leaves p[4..15] indeterminate: not reproduced.)  On the device plant the estimator, like
 * the EKF, is created with compensate_coef = rotor_constant = 1 (see brov_ekf_apply_to_solver). */
int brov_rls_apply_to_solver(brov_rls* r, brov_solver* s, int mode, void* stream);
/* outputs of the last tick; NULL skips.  status 0 ok, 2 non-finite theta or P (a NaN input propagates as in the reference, in its
 * own instance only) */
int brov_rls_get_outputs_host(brov_rls* r, double* mpc_p /*[B][4]*/, double* wf_env /*[B][6]*/, int* status /*[B]*/);
const double* brov_rls_theta_device(const brov_rls* r);   /* DEVICE theta, [4 components][B][4 axes] */
/* seconds of the last update kernel (HIP events on its stream) */
int brov_rls_last_update_seconds(brov_rls* r, double* seconds);

/* ---- the DOB / AMPC control loop on the device: the counterpart of brov_closed_loop with the observer in the loop.  Per tick k it
 * enqueues, on one stream (the solver's last one), exactly
 *     brov_set_yref_from_traj(s, line0 + k, ncols)
 *     brov_solve(s)
 *     brov_plant_step(s, dt, substeps)                  under the wrench mode in force (brov_plant_wrench_*)
 *     brov_ekf_update_from_solver(e, s)
 *     r == NULL (the DOB node):   brov_ekf_apply_to_solver(e, s)
 *     else (the AMPC node):       brov_rls_update_from_ekf(r, e, s);  brov_rls_apply_to_solver(r, s, rls_mode)      (bluerov2_ampc.cpp:346-349)
 * and waits on the host ONCE, at the end.  The results are bit-identical to that call sequence.  Optional HOST logs: u_log [ticks][B][4],
 * x_log [ticks+1][B][12], st_log [ticks][B], w_log [ticks][B][6] as brov_closed_loop_ex; est_log [ticks][B][6]: the observer's disturbance
 * estimate x[12..17] after each tick.  The three objects must hold the same batch (BROV_ERR_ARG otherwise).  An error of one of the calls
 * inside ends the loop and is returned with that call's own code (its text through brov_last_error); the logs are delivered only when the
 * whole loop succeeded, and the tick counter and the objects' states then stand where the failing tick left them. */
int brov_closed_loop_dob(brov_solver* s, brov_ekf* e, brov_rls* r /*NULL: DOB; else AMPC*/, int rls_mode, int ticks, int line0, int ncols,
                         double dt, int substeps, double* u_log, double* x_log, int32_t* st_log, double* w_log, double* est_log);

/* ---------------------------------------------------------------------------------------------------------------------
 * Batched tracking statistics: closed loops scored on the device.  What users do with the logs of a closed loop is always the same
 * reduction -- the RMS position error against the trajectory (the reference's bluerov2_states/scripts/error.py) --
 * and at Monte-Carlo batch sizes the logs themselves are the bottleneck.  A brov_track holds one 96-byte record
 * per instance, fed from logs [K][B][..] of K consecutive ticks; the record is updated in tick order, so it does not depend on how a
 * run is cut into calls (bit for bit).  Ticks are numbered from the last brov_track_reset: tick number = ticks + nonfinite so far.
 *   counted tick    x, y, z, psi of the state row (columns 0, 1, 2, 5: the only ones read) and the four inputs are all finite.
 *                   e2 = ((x-xr)^2 + (y-yr)^2) + (z-zr)^2 and the other squares in plain IEEE arithmetic in this order (no fused
 *                   multiply-add): sums and maxima equal a sequential restatement bit for bit (tests/track_restatement.py)
 *   non-finite tick any of those eight values is NaN or +-Inf: counted in `nonfinite`, in `failed` / `first_failed` if its status says so,
 *                   and in nothing else -- it reaches neither the sums nor the maxima
 * The yaw error is the raw difference psi - psi_r, NOT wrapped to (-pi, pi]: the OCP's residual is the unwrapped difference too, and
 * trajectory and plant state are both continuous in yaw (the circle's psi grows past pi without a jump), so wrapping would score a
 * state that the controller sees as a full turn off as on target.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct brov_track_stats {
    double  sum_pos2;       /* sum over counted ticks of e2 */
    double  sum_yaw2;       /* sum of (psi - psi_r)^2 */
    double  max_pos2;       /* max of e2 (squared: the host takes the root) */
    double  max_yaw;        /* max |psi - psi_r| */
    double  sum_u2[BROV_NU];/* sum of u_c^2 */
    int32_t ticks;          /* counted ticks */
    int32_t failed;         /* ticks with status != 0 (counted or not) */
    int32_t saturated;      /* counted ticks with any u_c <= lbu_c or u_c >= ubu_c */
    int32_t nonfinite;      /* non-finite ticks */
    int32_t first_failed;   /* number of the first tick with status != 0; -1: none */
    int32_t worst_tick;     /* number of the tick that set max_pos2, the first such tick on ties; -1 while ticks == 0 */
    int32_t pad_[2];        /* zero */
} brov_track_stats;
/* the whole batch.  Instances with ticks == 0 add nothing to the sums and cannot be the worst instance (their failed / nonfinite
 * counts are totalled: an instance that was NaN from its first tick on shows there); no counted tick at all: rms = 0, worst_instance = -1 */
typedef struct brov_track_summary {
    double  rms_pos;        /* sqrt(sum of sum_pos2 / sum of ticks) */
    double  rms_yaw;        /* sqrt(sum of sum_yaw2 / sum of ticks) */
    double  worst_max_pos2; /* the largest max_pos2 of the batch */
    int64_t ticks, failed, saturated, nonfinite;   /* totals */
    int32_t worst_instance; /* where worst_max_pos2 sits, the lowest index on ties */
    int32_t failed_instances;   /* instances with failed > 0 */
} brov_track_summary;
typedef struct brov_track brov_track;
typedef struct brov_track_params {   /* input bounds that `saturated` is judged by */
    double lbu[BROV_NU], ubu[BROV_NU];
} brov_track_params;
void brov_track_default_params(brov_track_params* p);   /* the bounds of brov_default_opts */
const char* brov_track_last_error(void); /* message of the last failing brov_track_* call on this thread */
int  brov_track_create(brov_track** out, int device, int batch, const brov_track_params* p /* NULL: defaults */);
void brov_track_destroy(brov_track* t);
int  brov_track_batch(const brov_track* t);
int  brov_track_reset(brov_track* t);   /* every record: zeros, first_failed = worst_tick = -1 */
/* K >= 1 ticks of logs x [K][B][12], u [K][B][4], status [K][B] (NULL: all zero) against the trajectory table ref [rows][16]: tick j of
 * the call is compared with row min(line1 + j, rows - 1) (rows below 0: row 0).  HOST pointers: copied, then one kernel.  DEVICE
 * pointers: one kernel enqueued on `stream`, no host wait; the logs must stay valid until it has run. */
int brov_track_accumulate_host(brov_track* t, const double* x, const double* u, const int32_t* status, int K, const double* ref, int rows,
                               int line1);
int brov_track_accumulate_device(brov_track* t, const double* x, const double* u, const int32_t* status, int K, const double* ref, int rows,
                                 int line1, void* stream);
int brov_track_get_stats_host(brov_track* t, brov_track_stats* stats /*[B]*/);
/* reduced on the device without floating-point atomics, in an order that depends on the batch size only: two calls return the same bytes */
int brov_track_get_summary_host(brov_track* t, brov_track_summary* summary);
/* seconds of the last accumulate kernel (HIP events on its stream) */
int brov_track_last_seconds(brov_track* t, double* seconds);
/* A closed loop that is scored instead of logged.  e == NULL: the ticks of brov_closed_loop_ex (the one-launch kernel where that call would
 * take it for the whole run, a launch per tick otherwise, e.g. under a wrench mode); with an observer: the ticks of brov_closed_loop_dob
 * (r == NULL: DOB, else AMPC with rls_mode).  The run is cut into chunks of `chunk` ticks (0: 64; < 0: BROV_ERR_ARG); each chunk writes
 * DEVICE logs sized for ONE chunk -- the same buffers for every chunk -- and is followed on the same stream by one accumulate against the
 * solver's own trajectory table: the state after tick k against row min(line0 + k + 1, rows - 1), saturation judged by the solver's bounds
 * of the moment (brov_opts::lbu / ubu).  One host wait, at the end; no host log.  Solver, observer and estimator end bit for bit where
 * the loop they mirror leaves them.  The record is NOT reset: successive calls continue the same statistics.  The objects must hold the
 * same batch (BROV_ERR_ARG); otherwise arguments and errors are those of the mirrored loop (text through brov_last_error). */
int brov_closed_loop_track(brov_solver* s, brov_ekf* e /*NULL: no observer*/, brov_rls* r /*NULL: DOB; else AMPC*/, int rls_mode, brov_track* t,
                           int ticks, int line0, int ncols, double dt, int substeps, int chunk);

/* ---------------------------------------------------------------------------------------------------------------------
 * Fleet planning loop: per-vehicle candidate selection on the device (BASELINE config 4 as a planner).
 * A fleet is V vehicles x C candidates laid over ONE brov_solver of batch B = V * C: instance b = v * C + c is candidate c of vehicle v,
 * and all candidates of a vehicle share that vehicle's measured state xv[v].  One planning tick: the candidates' windows are built
 * (brov_set_yref_candidates), all B candidates are solved in one launch (brov_solve), and brov_fleet_step
 *   selects  per vehicle the eligible candidate of the lowest cost, the lowest index on equal cost; eligible = status SUCCESS and a finite
 *            cost (NaN and +-Inf never win); winner = its index c within the group, -1 when the group has no eligible candidate
 *   steps    the vehicle's plant -- the ERK4 of brov_plant_step -- with the winner's u0 and the vehicle's true parameters, under the
 *            vehicle's world-frame wrench of this tick when a mode of brov_vehicle_wrench_* is in force.  Without a winner
 *            the vehicle is stepped with the input it was given last (zeros after brov_fleet_reset): the zero-order hold brov_opts::on_failure
 *            documents for one instance.  Logged status: 0 with a winner; without one the status of candidate 0 of the group if that is
 *            non-zero, else BROV_STATUS_NAN (candidate 0 reported success with a cost that is not finite)
 *   measures the new xv[v] becomes x0 of every candidate of vehicle v
 * With a disturbance observer of batch V the tick goes on: brov_vehicle_observe feeds it the vehicles' measurements, and
 * brov_vehicle_apply_estimate hands its estimate to all candidates of each vehicle; brov_closed_loop_fleet_dob is the whole loop.
 * The candidates' iterates are left alone: each candidate warm-starts from its own last step (the iterate is not shifted).  The fleet does
 * not own the solver, which must outlive it; the solver's x0 is the fleet's to write once a step has run.
 * Disturbance is a property of the VEHICLE, so it is the fleet's: the solver's own wrench (brov_plant_wrench_*) is indexed by the instance
 * v * C + c and means nothing here, and the 6-disturbance variant has no per-vehicle source.  brov_fleet_step and the fleet's loops fail with
 * BROV_ERR_ARG while either is in force on the solver, and the loops also when no candidate parameters were uploaded
 * (brov_set_candidate_params_host).  Every enqueueing call is ordered behind the solver's last stream (brov_order_stream) and behind the
 * fleet's own last work.
 * ------------------------------------------------------------------------------------------------------------------- */
typedef struct brov_fleet brov_fleet;
const char* brov_fleet_last_error(void); /* message of the last failing brov_fleet_* / brov_closed_loop_fleet call on this thread */
int  brov_fleet_create(brov_fleet** out, brov_solver* s, int candidates);   /* B % candidates == 0, 1 <= candidates <= B; else BROV_ERR_ARG */
void brov_fleet_destroy(brov_fleet* f);                                      /* does not destroy the solver */
int  brov_fleet_vehicles(const brov_fleet* f);
int  brov_fleet_candidates(const brov_fleet* f);
int  brov_fleet_reset(brov_fleet* f);                    /* u_hold = 0; v_prev = 0; xv := x0 of candidate 0 of every group; tick counter 0; Gauss-Markov current := its mean; plan and clearance statistics as new (done by create) */
int  brov_fleet_set_state_host(brov_fleet* f, const double* xv /*[V][12]*/);   /* also broadcast into the solver's x0 */
int  brov_fleet_get_state_host(brov_fleet* f, double* xv /*[V][12]*/);
int  brov_fleet_set_plant_params_host(brov_fleet* f, const double* p /*[V][16]; NULL: stage-0 parameters of candidate 0 of each group, re-read at every step*/);
/* segmented select alone.  rec: DEVICE [B] records, NULL = the solver's own (brov_results_device).  winner DEVICE [V], winner_rec DEVICE [V] or
 * NULL: a copy of the winning record, zeros where winner == -1.  Two calls on the same records return the same bytes. */
int  brov_fleet_select_device(brov_fleet* f, const brov_result* rec, int32_t* winner, brov_result* winner_rec, void* stream);
int  brov_fleet_select_host(brov_fleet* f, const brov_result* rec_host /*[B] or NULL*/, int32_t* winner /*[V]*/, brov_result* winner_rec /*[V] or NULL*/);
/* select + plant + broadcast from the given records (DEVICE [B]; NULL = the solver's).  Callers that re-score candidates
 * (e.g. add a penalty to `cost`) pass their own records; the re-scoring that keeps the vehicles apart is done on the device
 * (brov_clearance_set below): with it on, the step re-scores the records it is given, selects, and publishes the winners' paths. */
int  brov_fleet_step(brov_fleet* f, const brov_result* rec, double dt, int substeps, void* stream);
/* of the last step, HOST, any may be NULL: the input every vehicle was given u [V][4], its status [V] and its winner [V] */
int  brov_fleet_get_last_host(brov_fleet* f, double* u, int32_t* status, int32_t* winner);
/* `ticks` planning ticks, one host wait at the end.  Per tick k: brov_set_yref_candidates(s, t0 + k*dt_ref, dt_node) -> brov_solve(s) -> brov_fleet_step
 * (under the fleet's wrench mode), on the solver's last stream, from the solver's x0 as it stands (brov_fleet_reset / brov_fleet_set_state_host make it the fleet's xv).
 * HOST logs, any may be NULL: u_log [ticks][V][4], x_log [ticks+1][V][12], st_log [ticks][V], win_log [ticks][V] -- the layouts of
 * brov_track_accumulate_host at batch V.  Logs are delivered only when the whole loop succeeded (the contract of brov_closed_loop_ex). */
int  brov_closed_loop_fleet(brov_fleet* f, int ticks, double t0, double dt_ref, double dt_node, double dt, int substeps,
                            double* u_log, double* x_log, int32_t* st_log, int32_t* win_log);
/* seconds of the last select kernel (HIP events on its stream) */
int  brov_fleet_last_seconds(brov_fleet* f, double* select_seconds);

/* ---- the fleet under disturbance.  (These calls take a brov_fleet and act per vehicle; brov_fleet_last_error() has their texts.) -----------
 * A world-frame wrench per vehicle: brov_plant_wrench_* at batch V, owned by the fleet.  The generator is the solver's, with the vehicle v as
 * its instance index: vehicle v draws what instance v of a solver of batch V draws under the same settings.  The tick counter counts fleet
 * steps: +1 in every brov_fleet_step and in every tick of the fleet's loops, whatever the mode; brov_fleet_reset sets it to 0,
 * brov_vehicle_wrench_seek to `tick`.  Arguments are checked as the solver's are (tz_div != 0, rows >= 1, the periodic half-period index of
 * every tick a call will touch below 2^22: a step or a loop that would leave that range is refused before anything runs) -- both families go
 * through one function, so a refusal of either has BROV_ERR_ARG and a text that begins with the entry point's name.  The constant and
 * table buffers are copies the fleet keeps until the next upload.  Mode OFF (the default): brov_fleet_step launches the plant kernel it
 * always launched. */
int brov_vehicle_wrench_constant_host(brov_fleet* f, const double* w /*[V][6]*/);
int brov_vehicle_wrench_periodic(brov_fleet* f, uint64_t seed, double scale, double phase0, double dphi, double tz_div);
int brov_vehicle_wrench_table_host(brov_fleet* f, const double* tab /*[rows][6]*/, int rows, const double* gain /*[V] or NULL*/);
int brov_vehicle_wrench_off(brov_fleet* f);
int brov_vehicle_wrench_mode(const brov_fleet* f);             /* BROV_WRENCH_*; OFF for NULL */
int brov_vehicle_wrench_seek(brov_fleet* f, int64_t tick);     /* tick >= 0 */
int64_t brov_vehicle_wrench_tick(const brov_fleet* f);
/* the wrench of every vehicle at `tick`, HOST [V][6]; moves neither the counter nor a state; zeros while OFF */
int brov_vehicle_wrench_eval_host(brov_fleet* f, int64_t tick, double* w /*[V][6]*/);
/* The water the vehicles move in: the ocean current (brov_current_*) and the Coriolis stage (brov_coriolis_*) at batch V, owned by the fleet,
 * with the vehicle v as the instance index: vehicle v is in the current, and draws the Gauss-Markov noise, of instance v of a solver of batch V
 * under the same settings, whatever C.  Semantics, argument checks and refusals are those of the solver's two families (BROV_ERR_ARG, a text
 * in brov_fleet_last_error() that starts with the call's name; nothing changes, nothing is waited for).  The plant tick is the fleet's step
 * counter, the one brov_vehicle_wrench_tick reads; a Gauss-Markov step or loop that would draw at a tick >= 2^22 is refused before anything
 * is enqueued.  A TABLE current with a per-vehicle gain is the case of ONE body of water and V vehicles in it: one time series, scaled by what
 * each vehicle sees of it.  The added masses of the Coriolis stage are the vehicle's true parameters p[4..6] (brov_fleet_set_plant_params_host),
 * or, without them, the stage-0 parameters of candidate 0 the fleet's plant reads.
 * With a current mode in force or the Coriolis stage on, brov_fleet_step and the fleet's loops launch fleet_plant_water_kernel in place of
 * their plant kernel: the current is evaluated inside it (no launch more per tick), the wrench mode in force stays on top.  With both off (the
 * default) every launch is the one of a fleet without them.  brov_fleet_reset sets the Gauss-Markov state back to its mean, as it sets the
 * counter to 0, and zeroes what the two _last_host calls return; modes and settings stay in force, as the wrench's do.  The observer
 * (brov_vehicle_observe, brov_vehicle_apply_estimate) sees the water only through the vehicles' motion.  The solver's OWN current and Coriolis
 * stage are indexed by the instance v * C + c and stay refused by the fleet's step and loops.
 * The two families are declared in bluerov2_nmpc_water.h, which this header includes here: every caller of this header has them. */
#include "bluerov2_nmpc_water.h"
/* The observer's tick behind a fleet step, brov_ekf_batch(e) == V: measurement = xv, thrusts = the reference's allocation of the input every
 * vehicle was GIVEN in the last step (the winner's u0 or the held input) with the OCP model's rotor constant, acceleration = (v - v_prev) / dt
 * with v_prev kept in the fleet (zeros after brov_fleet_reset); then brov_ekf_update_device on `stream`.  `dt` is the time between two
 * measurements, i.e. the loop's plant period; brov_ekf_update_from_solver divides by the observer's own brov_ekf_params::dt instead -- the
 * two agree when the two are equal. */
int brov_vehicle_observe(brov_fleet* f, brov_ekf* e, double dt, void* stream);
/* p[0..3] of every stage of every candidate of vehicle v := brov_ekf_mpc_p_device(e)[v]; p[4..15] are left alone.  Same stream as the
 * brov_vehicle_observe of the tick.  BROV_ERR_ARG while the fleet's plant parameters are unset (brov_fleet_set_plant_params_host): the
 * fleet's plant would read the estimate back out of the controller's stage-0 parameters.  The observer is created with compensate_coef =
 * rotor_constant = 1 (see brov_ekf_apply_to_solver). */
int brov_vehicle_apply_estimate(brov_fleet* f, brov_ekf* e, void* stream);
/* brov_closed_loop_fleet under the fleet's wrench mode with the observer closing the loop.  Per tick k, on the solver's last stream:
 * brov_set_yref_candidates(s, t0 + k*dt_ref, dt_node) -> brov_solve(s) -> brov_fleet_step -> with e: brov_vehicle_observe(f, e, dt) ->
 * brov_vehicle_apply_estimate(f, e); one host wait at the end.  Logs as brov_closed_loop_fleet, and w_log HOST [ticks][V][6] or NULL: the
 * wrench every vehicle was under (zeros while OFF), est_log HOST [ticks][V][6] or NULL: the observer's x[12..17] after each tick.
 * e == NULL: brov_closed_loop_fleet with the wrench log; est_log must then be NULL.  With e the refusals of brov_vehicle_apply_estimate hold. */
int brov_closed_loop_fleet_dob(brov_fleet* f, brov_ekf* e /*NULL: no observer*/, int ticks, double t0, double dt_ref, double dt_node,
                               double dt, int substeps, double* u_log, double* x_log, int32_t* st_log, int32_t* win_log,
                               double* w_log /*[ticks][V][6]*/, double* est_log /*[ticks][V][6]*/);

/* ---- the inter-vehicle clearance term.  (These calls take a brov_fleet; brov_fleet_last_error() has their texts.) ----
 * The fleet owns a PLAN per vehicle, plan [V][N+1][3]: the positions x, y, z of the path the vehicle committed to last.  After
 * brov_fleet_create, brov_fleet_reset and brov_fleet_set_state_host every stage of plan[v] is the position of xv[v] (the vehicle stays where
 * it is).  With the term on (brov_clearance_set; off by default, and then every call launches exactly what it launched before), brov_fleet_step
 * and every tick of the fleet's loops run
 *   clearance  d2min[b], b = v * C + c: the minimum over the peers w != v and the stages k = 0..N of ((dx*dx + dy*dy) + dz*dz) with
 *              d = x[b][k][0..2] - plan[w][min(k + shift, N)], x the solver's iterate; every operation rounded on its own; the minimum starts
 *              at +Inf and is updated by d2 < m, so a NaN distance is skipped; V = 1 gives +Inf.  Two calls return the same bytes.
 *   re-score   into records the fleet owns: a copy of every record, with cost := cost + weight * (r2 - d2min[b]) where d2min[b] < r2 =
 *              radius * radius (three operations, each rounded; a cost that is NaN already keeps its bytes, a NaN the sum generates, -Inf + Inf,
 *              is written as the quiet NaN 0x7ff8000000000000).
 *              weight = +Inf makes the term a hard constraint: the cost becomes +Inf, which the select treats as ineligible
 *   the select, the plant and the broadcast of brov_fleet_step on the re-scored records (a vehicle whose candidates were all priced out holds
 *              its input, with the logged status of that rule)
 *   publish    with a winner c, plan[v][k] := x[v*C+c][k][0..2] for k = 0..N; without one the old plan advances by `shift` stages,
 *              plan[v][k] := plan[v][min(k + shift, N)].  Statistics per vehicle, reset where the plan is: last_d2 = d2min of this step's
 *              winner or -1.0 without one (and before the first step), min_d2 = the minimum of last_d2 over the steps that had a winner (+Inf
 *              before the first), below = the number of steps whose winner had d2min < r2
 * Steps with the term off leave plan and statistics alone; brov_clearance_off keeps the plan, the statistics and the parameters. */
int brov_clearance_set(brov_fleet* f, double radius, double weight, int shift);
        /* radius finite > 0 with radius * radius finite and > 0 (about 1.5e-162 < radius < 1.3e154), weight > 0 (may be +Inf, not NaN),
         * 0 <= shift <= N; else BROV_ERR_ARG */
int brov_clearance_off(brov_fleet* f);
int brov_clearance_enabled(const brov_fleet* f);                      /* 0 for NULL */
int brov_clearance_set_plan_host(brov_fleet* f, const double* plan /*[V][N+1][3]*/);
int brov_clearance_get_plan_host(brov_fleet* f, double* plan);
/* the two kernels alone, against the plan as it stands (moves nothing): x DEVICE [B][N+1][12] or NULL = brov_x_device(solver),
 * rec DEVICE [B] or NULL = the solver's records; d2min DEVICE [B]; out DEVICE [B] or NULL.  BROV_ERR_ARG while the term is off: radius,
 * weight and shift come from brov_clearance_set.  Ordered behind the solver's last stream and the fleet's own last work. */
int brov_clearance_eval_device(brov_fleet* f, const double* x, const brov_result* rec, double* d2min, brov_result* out, void* stream);
int brov_clearance_eval_host(brov_fleet* f, const brov_result* rec_host /*[B] or NULL*/, double* d2min /*[B]*/, brov_result* out /*[B] or NULL*/);
int brov_clearance_get_stats_host(brov_fleet* f, double* last_d2, double* min_d2, int32_t* below /*[V] each, any NULL*/);
int brov_clearance_last_seconds(brov_fleet* f, double* seconds);      /* the distance kernel, HIP events */
/* development and tests: into how many grid-level slices the distance kernel cuts the peer range (1..8; 0: the default, chosen from B and V).
 * A tuning knob only: d2min is a minimum, its bytes do not depend on the count -- which is what the tests hold with it. */
int brov_clearance_dev_set_slices(brov_fleet* f, int slices);
int brov_clearance_dev_slices(const brov_fleet* f);                   /* the count in force; 0 for NULL */

/* ---------------------------------------------------------------------------------------------------------------------
 * The reference's second disturbance observer: the 21-dimensional error-state Kalman filter over IMU and GPS of the bluerov2_states
 * nodelet, brov_eskf_* (DESIGN.md section 4.4b).  Declared in bluerov2_nmpc_eskf.h, which this header includes here.
 * ------------------------------------------------------------------------------------------------------------------- */
#include "bluerov2_nmpc_eskf.h"
/* The IMU/GPS stage of the solver's plant, brov_imu_*, and the filter at its sensors' own rates: the masked tick brov_imu_eskf_tick_*, the hand-off
 * brov_imu_eskf_tick_from_solver and the loop brov_closed_loop_eskf (DESIGN.md sections 4.9h and 4.4c).  Declared in bluerov2_nmpc_imu.h. */
#include "bluerov2_nmpc_imu.h"
/* The bridge-pier inspection loop of the reference's third demo: the depth camera's mean range against scene geometry, brov_range_*, the
 * mission machine with its three PID loops, brov_inspect_*, and the loop brov_closed_loop_inspect.  Declared in
 * bluerov2_nmpc_inspect.h. */
#include "bluerov2_nmpc_inspect.h"
/* The thrust-curve stage of the solver's plant, brov_curve_*: the controller's command map and the ESC's steps ahead of the rotor stage, the
 * speed-to-thrust conversion (quadratic, dead-zone quadratic or a measured table with its current draw) and an efficiency behind it
 * (DESIGN.md section 4.9j).  Declared in bluerov2_nmpc_curve.h. */
#include "bluerov2_nmpc_curve.h"
/* Triangle meshes in the scene of the range stage, brov_mesh_*: a world-frame mesh beside the boxes, a Moeller-Trumbore test restated bit for
 * bit, and a skip-link bounding-volume hierarchy whose only contract is the result of testing every triangle.
 * Declared in bluerov2_nmpc_mesh.h. */
#include "bluerov2_nmpc_mesh.h"
/* The stand-off term of the fleet loop, brov_standoff_*: every candidate priced by the closest approach of its predicted path to the scene of
 * the range stage, mesh and boxes, ahead of the select.  Declared in bluerov2_nmpc_standoff.h. */
#include "bluerov2_nmpc_standoff.h"

#ifdef __cplusplus
}
#endif
#endif
