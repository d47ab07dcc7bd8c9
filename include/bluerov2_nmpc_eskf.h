/* bluerov2_nmpc_eskf.h -- brov_eskf_*: B independent copies of the reference's second disturbance observer, the error-state Kalman filter over
 * IMU and GPS of the bluerov2_states nodelet (src/Eskf.cpp, Dynamics.cpp, Config.cpp), whose last three states are a body-frame disturbance
 * force xi and which publishes /disturbance.  Part of the C ABI of bluerov2_nmpc.h, which includes this file behind its EKF and RLS sections;
 * not meant to be included on its own.
 *
 * Nominal state per instance, FP64, x[22] = [p_I(3) | v_I(3) | q(4: w, x, y, z) | b_g(3) | b_a(3) | g_I(3) | xi(3)].  Covariance P[21][21] over
 * the error state in the order the reference's F, H and Q use: [dp, dv, dtheta, db_g, db_a, dg, dxi] (the comment of ImuDo.h:153 gives another
 * order; the code counts).  P is taken as symmetric and comes back exactly symmetric.
 *
 * A tick.  q and q_meas are normalised on entry and every quaternion product is normalised (q / |q|).
 *   predict (Eskf.cpp:97-158), IMU sample imu = (a_m, w_m):  a = a_m - b_a, w = w_m - b_g, R = R(q) before the step;
 *     p += v dt + (R a) dt^2/2 + g_I dt^2/2;  v += (R a) dt + g_I dt  (old R; p uses the old v);  q = q * exp(w dt);
 *     F = I but F[3:6,6:9] = -R hat(a) dt, F[3:6,12:15] = -R dt (the NEW R), F[6:9,6:9] = exp(-w dt), F[0:3,3:6] = F[3:6,15:18] = I dt,
 *     F[6:9,9:12] = -I dt;  P = F P F' + diag(Q).
 *   update (:197-306):  y = [gps_p - p | gps_v - v | log(q^-1 * q_meas) | tau3 - (Mrb3 - xi + Ma3 + D3 + g3)], with the SAME IMU sample:
 *     Mrb3 = [m a0 + m ZG w1, m a1 - m ZG w0, m a2]  (M_rb times the bias-corrected IMU 6-vector, rates included, as the reference has it);
 *     Ma3_i = added_mass[i] (a_i + gB_i), gB = R(q_meas)' (0,0,-g)  (the MEASURED attitude);  D3_i = (-Dl[i] - Dnl[i] |vB_i|) vB_i, vB = R(q)' v;
 *     g3 = (m g - bouyancy) [sin th, -cos th sin ph, -cos th cos ph], roll and pitch of the estimated q;  tau3 = rows 0..2 of K thrust.
 *     H = 0 but H[0:3,0:3] = H[3:6,3:6] = H[6:9,6:9] = I, H[9:12,18:21] = -I;  S = H P H' + diag(R12), eliminated without row exchanges;
 *     Kal = P H' S^-1, dx = Kal y, P = (I - Kal H) P (the reference's simple form);
 *     p += dx[0:3]; v += vel_inject dx[3:6]; q = q * exp(dx[6:9]); xi += dx[18:21]; with inject_bias_g: b_g, b_a, g_I += dx[9:12], [12:15], [15:18].
 *   exp(phi) = [cos(|phi|/2), sin(|phi|/2) phi/|phi|], log(q) = 2 atan(|v|/w) v/|v| (Sophus' forms; below |.|^2 = 2^-40 their series).
 * Two quirks of the reference are parameters: vel_inject = 2 (Eskf.cpp:325 adds the velocity correction twice; 1 is the textbook filter) and
 * inject_bias_g = 0 (the reference never injects dx[9:18]).  Not reproduced: the debugging lines that overwrite the published disturbance with
 * a rotated constant (:83-87) -- the output is what the commented-out lines intended -- and the lat/lon-to-metres conversion: the API takes metres.
 *
 * Outputs per instance: xi; xi_world = R(q) xi; mpc_p = [xi0/compensate_coef, xi1/compensate_coef, xi2/rotor_constant, 0]
 * (bluerov2_dob_patty.cpp:355-358); status, with the meanings of brov_ekf_get_outputs_host: 0 ok; 1 a pivot of S is not positive or holds a
 * NaN -- state and covariance left at the prediction, the covariance exactly symmetric, the outputs made from it; 2 the estimate is not
 * finite.  A NaN in the IMU sample reaches S through F and gives 1; a NaN in the GPS position leaves S alone and gives 2.  A predict-only
 * tick gives 0 or 2. */
#ifndef BLUEROV2_NMPC_ESKF_H_
#define BLUEROV2_NMPC_ESKF_H_
#ifndef BLUEROV2_NMPC_H_
#error "include bluerov2_nmpc.h, which includes this file"
#endif

typedef struct brov_eskf brov_eskf;
typedef struct brov_eskf_params {
    double dt;             /* IMU period, 1/50 (Eskf.cpp:103) */
    double gps_dt;         /* GPS period, 1/30 (:184): only brov_eskf_update_from_solver divides by it */
    double mass, ZG, g, bouyancy;           /* ImuDo.h:101-110 */
    double added_mass[6], Dl[6], Dnl[6];    /* entries 0..2 are used */
    double K[36];          /* propulsion matrix, row-major (Config.cpp:175-180): rows 0..2 are used */
    double Q[21];          /* process noise, diagonal (Config.cpp:128-138: p,p,p, v,v,v, r,r,r, q x 9, xi,xi,xi; launch/config/imudo.yaml) */
    double R12[12];        /* measurement noise, diagonal (Config.cpp:147-154: p x 3, v x 3, r x 3, th x 3) */
    double vel_inject;     /* 2: the reference; 1: the textbook filter */
    double compensate_coef, rotor_constant; /* those of brov_ekf_params */
    int32_t inject_bias_g; /* 0: the reference; 1: dx[9:18] is injected into b_g, b_a, g_I */
    int32_t reserved;      /* 0 */
} brov_eskf_params;
void brov_eskf_default_params(brov_eskf_params* p);
const char* brov_eskf_last_error(void);   /* message of the last failing brov_eskf_* call on this thread */
/* refused with BROV_ERR_ARG and a text, before anything touches a device: batch <= 0, or a dt, gps_dt or R12 entry that is not positive */
int  brov_eskf_create(brov_eskf** out, int device, int batch, const brov_eskf_params* p /* NULL: defaults */);
void brov_eskf_destroy(brov_eskf* e);
int  brov_eskf_batch(const brov_eskf* e);
/* every instance := (x0, P0); NULL: x = 0 but q = (1,0,0,0) and g_I = (0,0,-g); P0 = 0 (ImuDo.h:155).  A q that is not finite or whose norm is
 * further than 1e-6 from 1 is refused (BROV_ERR_ARG), here and in brov_eskf_set_state_host, before anything is copied */
int brov_eskf_reset(brov_eskf* e, const double* x0 /*[22]*/, const double* P0 /*[21][21]*/);
int brov_eskf_set_state_host(brov_eskf* e, const double* x /*[B][22] or NULL*/, const double* P /*[B][21][21] or NULL*/);
int brov_eskf_get_state_host(brov_eskf* e, double* x /*[B][22] or NULL*/, double* P /*[B][21][21] or NULL*/);
/* a predict-only tick: the reference's branch when no GPS fix is due.  imu [B][6] = (a_m, w_m) */
int brov_eskf_predict_host(brov_eskf* e, const double* imu, void* stream);
int brov_eskf_predict_device(brov_eskf* e, const double* imu, void* stream);
/* predict followed by update.  imu [B][6], gps_p [B][3] metres, gps_v [B][3], q_meas [B][4] (w, x, y, z), thrust [B][6] */
int brov_eskf_update_host(brov_eskf* e, const double* imu, const double* gps_p, const double* gps_v, const double* q_meas, const double* thrust,
                          void* stream);
int brov_eskf_update_device(brov_eskf* e, const double* imu, const double* gps_p, const double* gps_v, const double* q_meas,
                            const double* thrust, void* stream);
int brov_eskf_get_outputs_host(brov_eskf* e, double* xi /*[B][3] or NULL*/, double* xi_world /*[B][3] or NULL*/, double* mpc_p /*[B][4] or NULL*/,
                               int* status /*[B] or NULL*/);
const double* brov_eskf_x_device(const brov_eskf* e);      /* [B][22] */
const double* brov_eskf_P_device(const brov_eskf* e);      /* [B][21][21] */
const double* brov_eskf_mpc_p_device(const brov_eskf* e);  /* [B][4] */
/* Closing the loop on the device.  brov_eskf_update_from_solver synthesises the filter's inputs from the state brov_ekf_update_from_solver reads
 * (the measured state while the solver's sensor stage is on, else the plant's) and the thrusts of the records that call reads, then runs the
 * update tick:  q_meas and R from the Euler angles;  v_I = R nu;  a_m = R'((v_I - v_I,prev)/dt - g_I), g_I = (0,0,-g);  w_m = (p,q,r);
 * gps_p = (x,y,z);  gps_v = (gps_p - gps_p,prev)/gps_dt.  The previous values are kept in the observer; the first call after brov_eskf_reset or
 * brov_eskf_set_state_host takes them equal to the current ones.  (The reference starts them at zero, which at a depth of 20 m makes the first
 * GPS velocity -20 m / gps_dt; this first tick therefore differs from the reference's.)
 * brov_eskf_apply_to_solver: p[0..3] of every stage of instance b := mpc_p of instance b; p[4..15] are left alone.  Units as for
 * brov_ekf_apply_to_solver: an observer that compensates the device plant is created with compensate_coef = rotor_constant = 1. */
int brov_eskf_update_from_solver(brov_eskf* e, brov_solver* s, void* stream);
int brov_eskf_apply_to_solver(brov_eskf* e, brov_solver* s, void* stream);
/* the inputs of the last update tick as the observer holds them (those brov_eskf_update_host copied, or brov_eskf_update_from_solver made) */
int brov_eskf_get_inputs_host(brov_eskf* e, double* imu /*[B][6] or NULL*/, double* gps_p /*[B][3] or NULL*/, double* gps_v /*[B][3] or NULL*/,
                              double* q_meas /*[B][4] or NULL*/, double* thrust /*[B][6] or NULL*/);
int brov_eskf_last_update_seconds(brov_eskf* e, double* seconds);   /* seconds of the last tick's kernel (HIP events on its stream) */

#endif
