/* bluerov2_nmpc_imu.h -- brov_imu_*: the IMU/GPS stage of a solver's plant, the sensor model of the error-state filter (brov_eskf_*), and the
 * filter run at its sensors' own rates: brov_imu_eskf_tick_*, brov_imu_eskf_tick_from_solver, brov_closed_loop_eskf.  The reference's nodelet predicts on
 * every IMU sample and updates only when a GPS fix has arrived (ImuDoNodelet::EskfProcess, bluerov2_states/src/Eskf.cpp:4-41); IMU and GPS run at
 * their own rates (:103, :184), both faster than the controller.  Part of the C ABI of bluerov2_nmpc.h, which includes this file behind
 * bluerov2_nmpc_eskf.h; not meant to be included on its own.
 *
 * The stage.  A seventh stage of the solver's plant, beside the sensor stage (brov_sensor_*), which measures the 12 states the NMPC sees; this
 * one makes what the filter reads and always reads the TRUE plant state.  No plant kernel changes: a regular refresh (imu_measure_kernel) runs
 * behind the plant kernel of every plant step, on the same stream, at the counter's new value m, the measurement index, which must stay in
 * [0, 2^24).  Per instance b, after a step of length h to the true state x = (p | phi theta psi | nu | p q r):
 *   R, q(phi, theta, psi) from the Euler angles, as brov_eskf_update_from_solver forms them;   v_I = R nu;
 *   a = R'((v_I - v_I,prev) / h - g_I), g_I = (0, 0, -g): the mean specific force of the step, what a delta-velocity IMU reports;  w = (p, q, r);
 *   a_m[k] = (a[k] + bias[b][k])     + sigma[b][k]     n(b, m, 16 + k)
 *   w_m[k] = (w[k] + bias[b][3 + k]) + sigma[b][3 + k] n(b, m, 19 + k)
 * every operation rounded on its own.  n is the sensor stage's counter-based Irwin-Hall(12) variate -- the same hash, salt and key layout -- at the
 * channel slots 16..28: a sensor stage and an IMU stage with the same seed draw from disjoint counters.
 * A fix is DUE iff m % gps_every == 0.  A due fix is DROPPED iff dropout[b] > 0 and the draw u = (H >> 11) 2^-53 at slot 28, j = 0, is below
 * dropout[b].  fix[b] = due and not dropped.  With a fix:
 *   gps_p[k] = x[k] + sigma[b][6 + k] n(b, m, 22 + k)
 *   gps_v    = (gps_p - gps_p,last) / (gps_every h)   the constant nominal period, as Eskf.cpp:184 has it: after a dropped fix the velocity is too
 *              large, as in the reference.  BROV_IMU_GPSV_ELAPSED divides by (m - m_last) h instead.
 *   q_meas   = q(phi, theta, psi) * exp(sigma[b][9..11] . n(b, m, 25..27)), normalised;   gps_p,last and m_last move.
 * Without a fix gps_p, gps_v and q_meas keep their values.  Statistics per instance: samples, fixes taken, fixes dropped.
 * A forced restart -- brov_imu_set_host (which first resets the statistics), brov_set_x0_host / brov_set_x0_device and brov_sensor_measure while
 * the stage is on, brov_imu_restart -- sets v_I,prev to the current v_I, so the acceleration is gravity alone, and takes a fix without a dropout
 * draw with gps_v = 0; the statistics are untouched.
 * While the stage is on: a plant step whose dt is not bit-equal to h is refused with BROV_ERR_ARG and steps nothing (the rotor stage's rule); the
 * closed loops take their launch-per-tick branch (the *_ticks kernels know no stage); the fleet's step and loops refuse the solver.  Stage off
 * (the default, and after brov_imu_off): no launch is added anywhere. */
#ifndef BLUEROV2_NMPC_IMU_H_
#define BLUEROV2_NMPC_IMU_H_
#ifndef BLUEROV2_NMPC_H_
#error "include bluerov2_nmpc.h, which includes this file"
#endif

#define BROV_IMU_GPSV_ELAPSED 1   /* gps_v divides by the time since the last fix taken, not by the nominal GPS period */
typedef struct brov_imu_params {
    double h;              /* the plant step the stage samples, seconds: > 0 */
    double g;              /* gravity, 9.81 */
    int32_t gps_every;     /* a fix is due every gps_every samples: >= 1 */
    int32_t flags;         /* BROV_IMU_* */
    uint64_t seed;
} brov_imu_params;
void brov_imu_default_params(brov_imu_params* p);   /* h = 0.01, g = 9.81, gps_every = 1, no flag, seed 0 */
/* The stage comes into force and restarts at the counter's index.  Refused with BROV_ERR_ARG and a text in brov_last_error(), before anything
 * touches a device: h <= 0, gps_every < 1, a negative or NaN sigma, a bias that is not finite, a dropout outside [0, 1] */
int brov_imu_set_host(brov_solver* s, const brov_imu_params* p, const double* sigma /*[B][12]: a, w, gps_p, attitude; NULL: 0*/,
                      const double* bias /*[B][6]: a, w; NULL: 0*/, const double* dropout /*[B]; NULL: 0*/);
int brov_imu_off(brov_solver* s);
int brov_imu_enabled(const brov_solver* s);                    /* 0 for NULL */
int brov_imu_restart(brov_solver* s, void* stream);            /* forced restart at the current index */
/* the stage alone: a regular refresh's sample at `index` for the given state, previous inertial velocity, last fix and its index (< 0: none,
 * gps_v = 0), with the configuration in force (before any brov_imu_set_host: the defaults).  Without a fix gps_p, gps_v and q_meas come back as
 * zeros.  It moves nothing and touches no statistic */
int brov_imu_eval_host(brov_solver* s, int64_t index, const double* x /*[B][12]*/, const double* v_prev /*[B][3]*/,
                       const double* gps_p_last /*[B][3]*/, const int32_t* m_last /*[B]*/, double* imu /*[B][6]*/, double* gps_p /*[B][3]*/,
                       double* gps_v /*[B][3]*/, double* q_meas /*[B][4]*/, int32_t* fix /*[B]; any output NULL*/);
/* the last sample and its flags as the stage holds them (zeros before the first) */
int brov_imu_get_host(brov_solver* s, double* imu, double* gps_p, double* gps_v, double* q_meas, int32_t* fix /*any NULL*/);
int brov_imu_get_stats_host(brov_solver* s, int32_t* stats /*[B][3]: samples, fixes taken, fixes dropped*/, int64_t* refreshes /*any NULL*/);
int brov_imu_reset_stats(brov_solver* s);
int brov_imu_last_seconds(brov_solver* s, double* seconds);    /* the measure kernel's last launch, HIP events */

/* The filter's calls on the stage's samples are named brov_imu_eskf_*: they take a brov_eskf and report through brov_eskf_last_error(), but the
 * exported brov_eskf_* family is exactly what bluerov2_nmpc_eskf.h declares, and stays so.
 * One filter launch for a batch in which only some filters have a fix (eskf_tick_masked_kernel).  fix [B]: with fix[b] != 0 filter b does
 * exactly the update tick of brov_eskf_update_*, with fix[b] == 0 exactly the predict-only tick of brov_eskf_predict_* -- state, covariance,
 * outputs and status bit for bit.  A filter without a fix reports status 0 or 2; nothing made from its gps_p, gps_v, q_meas or thrust reaches
 * anything (they may hold NaNs; the arrays must exist). */
int brov_imu_eskf_tick_host(brov_eskf* e, const double* imu, const double* gps_p, const double* gps_v, const double* q_meas, const double* thrust,
                        const int32_t* fix, void* stream);
int brov_imu_eskf_tick_device(brov_eskf* e, const double* imu, const double* gps_p, const double* gps_v, const double* q_meas, const double* thrust,
                          const int32_t* fix, void* stream);
/* The hand-off at the sensors' rates.  Requires the solver's IMU stage on and the filter's dt bit-equal to the stage's h (else BROV_ERR_ARG with
 * a text in brov_eskf_last_error()).  The filter reads the stage's last sample, its fix flags and the thrusts brov_eskf_update_from_solver would
 * read at that moment.  No fix was due at the sample's index: the predict-only kernel; a fix was due: the masked kernel with the stage's flags.
 * brov_eskf_get_inputs_host then returns what this tick read. */
int brov_imu_eskf_tick_from_solver(brov_eskf* e, brov_solver* s, void* stream);
const double* brov_imu_eskf_xi_world_device(const brov_eskf* e);   /* [B][3] */
/* The loop as one call.  Per control tick k, on the solver's last stream: brov_set_yref_from_traj(s, line0 + k, ncols) -> brov_solve(s) ->
 * imu_per_tick times { brov_plant_step(s, dt / imu_per_tick, 1) -> brov_imu_eskf_tick_from_solver(e, s) } -> brov_eskf_apply_to_solver(e, s); the
 * same record is held over the plant steps of a tick; one host wait at the end.  Results and logs are those of that sequence composed by the
 * caller.  Logs (HOST, any NULL): u_log [ticks][B][4], x_log [ticks + 1][B][12] (one row per control tick behind the start state), st_log
 * [ticks][B], w_log [ticks][B][6] (the wrench of the tick's last plant step), est_log [ticks][B][3] (xi_world after the tick's last filter
 * step), fix_log [ticks][imu_per_tick][B].  Errors as brov_closed_loop_dob (text in brov_last_error()).  Whatever the stages in force refuse of
 * those plant steps is refused here: the IMU and the rotor stage need h = dt / imu_per_tick; a delay counts plant steps. */
int brov_closed_loop_eskf(brov_solver* s, brov_eskf* e, int ticks, int line0, int ncols, double dt, int imu_per_tick, double* u_log, double* x_log,
                          int32_t* st_log, double* w_log, double* est_log, int32_t* fix_log);

#endif
