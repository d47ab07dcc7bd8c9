/* bluerov2_nmpc_curve.h -- brov_curve_*: the thrust-curve stage of the solver's plant: what stands between a wanted thrust and the force a
 * thruster gives, besides its lag.  The reference's simulated vehicle (bluerov2_environ/urdf/snippets.xacro) puts FirstOrder dynamics on the
 * command and then a Basic conversion on the lagged command, thrust = rotorConstant w |w|; the real vehicle has the measured T200 curve
 * (bluerov2_dobmpc/config/thrusters: 201 rows, PWM 1100 ... 1900 us in steps of 4 at 16 V) with a dead band from 1472 to 1528 us, -4.07 kgf at
 * full reverse against +5.25 kgf at full forward, an ESC that takes whole PWM steps and a current draw per operating point; the controller's
 * own command map (t200_thrust2gain_map.yaml) is a degree-4 polynomial.  Part of the C ABI of bluerov2_nmpc.h, which includes this file behind
 * bluerov2_nmpc_inspect.h; not meant to be included on its own.
 *
 * The chain becomes
 *     controller record -> delay -> [curve: COMMAND part] -> rotor -> [curve: THRUST part] -> thruster stage (clip / fault / K) -> model
 * The COMMAND part is what the controller's side does to a wanted thrust before it leaves for the ESC: a pre-map and a quantisation.  The
 * THRUST part is what the thruster does with the lagged command: the conversion curve and an efficiency.  Dynamics on the command, then
 * conversion: the uuv plugin's order.  With the rotor stage off the two parts are adjacent and run as ONE launch (BOTH); with it on COMMAND
 * runs ahead of rotor_shift_kernel and THRUST behind it.  BOTH is DEFINED as COMMAND followed by THRUST, bit for bit, the rewritten u0 included.
 *
 * Per instance b and thruster i, t = thrust[i] of the record received; every operation is rounded on its own, there is no device
 * transcendental, division or reciprocal.
 * COMMAND part.  Pre-map: w = t (BROV_CURVE_PRE_NONE);  w = (((p0 t + p1) t + p2) t + p3) t + p4, Horner over pre_poly[5], highest degree
 *   first, the layout of numpy's polyfit and of the reference's yaml (BROV_CURVE_PRE_POLY);  w = lookup(pre table, t) (BROV_CURVE_PRE_TABLE).
 *   Quantisation: for quantum > 0, w = quantum * rint(w * inv_quantum), inv_quantum = 1 / quantum computed on the host, rint with ties to even.
 * THRUST part.  Conversion: f = w (BROV_CURVE_LINEAR: a copy that keeps the sign of zero);  f = k * (w * |w|) (BROV_CURVE_BASIC, the
 *   reference's vehicle);  with v = w * |w|:  f = kl * (v + (-dl)) for v <= dl, kr * (v + (-dr)) for v >= dr, +0.0 between
 *   (BROV_CURVE_DEADZONE);  f = lookup(curve table, w) (BROV_CURVE_TABLE).  Efficiency: f = eff[b][i] * f unless eff[b][i] == 1.0, which copies.
 *   eff carries the per-instance spread (battery voltage, a fouled propeller, the plugin's thrust_efficiency) and the unit change from the
 *   table's ordinate to what K multiplies.
 * Lookup, one routine for both tables.  Knots x[0..K) strictly increasing and finite, 2 <= K <= 256, ordinates y[K]; the slopes
 *   (y[j+1] - y[j]) / (x[j+1] - x[j]) are computed on the HOST in doubles and uploaded (slope[K-1] = 0); brov_curve_get_table_host hands back
 *   exactly the uploaded values.  w <= x[0] gives y[0] and w >= x[K-1] gives y[K-1], so +-inf clamps to the end knots; otherwise j is the
 *   largest index with x[j] <= w and the value is y[j] + slope[j] * (w + (-x[j])).  The curve table may carry a third column amps,
 *   interpolated with the same j and the same expression.
 * NaN.  A NaN that enters a part leaves it with its bits, whatever the modes (and its amps are that NaN); a NaN a part makes of another
 *   input (0 * inf, inf - inf) is the one quiet NaN 0x7FF8000000000000, so that the result does not depend on whose arithmetic made it.
 * Records.  A part that changes the bits of any of the six values writes thrust = its output and u0 = the allocation's left inverse of its
 *   output, in the operation order written in rotor_kernel.hip, so that the plant without the thruster stage and the observer see the
 *   delivered forces; a part that changes no bit copies the record whole.  The u log keeps the COMMANDED u0, written by the first stage of
 *   the chain that runs.
 * Books per plant step.  wanted = the t that entered the COMMAND part; last_command = w and last_thrust = f of the last step;
 *   err_sq[b] += sum_i (wanted_i - f_i)^2, the six squares summed in index order and added once into the sum;
 *   dead_ticks[b][i] += (f_i == 0 and wanted_i != 0);  with an amps column in BROV_CURVE_TABLE, charge[b] += dt * sum_i amps_i in A s with the
 *   step's own dt;  the stage's own step count.
 * observer_applied != 0: brov_ekf_update_from_solver reads this stage's applied records, ahead of the rotor's and the delay's flag.
 * Bit-reproducible against tests/curve_restatement.py.  The one-launch closed loop and the *_ticks kernels know no curve, so the loops take
 * their launch-per-tick branch; a brov_fleet refuses such a solver.  Stage off (the default, and after brov_curve_off): every launch is the
 * one of a solver without the stage.
 * Refused with BROV_ERR_ARG and a text in brov_last_error() that starts with the call's name (nothing changes, nothing is waited for): a NULL
 * handle; K outside [2, 256]; knots not strictly increasing; a non-finite table value or slope, eff, k, kl, kr, dl, dr or polynomial
 * coefficient; dl > dr; a negative or non-finite quantum; an unknown kind, pre, part or table; a table mode with no table set. */
#ifndef BLUEROV2_NMPC_CURVE_H_
#define BLUEROV2_NMPC_CURVE_H_
#ifndef BLUEROV2_NMPC_H_
#error "include bluerov2_nmpc.h, which includes this file"
#endif

#define BROV_CURVE_LINEAR 0
#define BROV_CURVE_BASIC 1
#define BROV_CURVE_DEADZONE 2
#define BROV_CURVE_TABLE 3
#define BROV_CURVE_PRE_NONE 0
#define BROV_CURVE_PRE_POLY 1
#define BROV_CURVE_PRE_TABLE 2
#define BROV_CURVE_PART_COMMAND 1
#define BROV_CURVE_PART_THRUST 2
#define BROV_CURVE_PART_BOTH 3
#define BROV_CURVE_WHICH_CURVE 0
#define BROV_CURVE_WHICH_PRE 1
#define BROV_CURVE_MAX_KNOTS 256

typedef struct brov_curve_params {
    int32_t kind;              /* BROV_CURVE_LINEAR ... BROV_CURVE_TABLE */
    int32_t pre;               /* BROV_CURVE_PRE_NONE ... BROV_CURVE_PRE_TABLE */
    double quantum;            /* step of the command behind the pre-map; 0: none */
    double k;                  /* BROV_CURVE_BASIC */
    double kl;                 /* BROV_CURVE_DEADZONE: slope left of the dead zone */
    double kr;                 /* ... and right of it */
    double dl;                 /* the dead zone of v = w |w|: dl <= dr */
    double dr;
    double pre_poly[5];        /* BROV_CURVE_PRE_POLY, highest degree first */
    int32_t observer_applied;
    int32_t reserved_;
} brov_curve_params;
/* LINEAR, PRE_NONE, quantum 0 -- a copy --, k = kl = kr = 1, dl = dr = 0, pre_poly the identity (0, 0, 0, 1, 0), observer_applied 0 */
void brov_curve_default_params(brov_curve_params* p);
/* a table of K knots for `which` (BROV_CURVE_WHICH_*); amps [K] or NULL, the curve table's alone.  It holds from the next plant step on; the
 * books stay */
int brov_curve_set_table_host(brov_solver* s, int32_t which, const double* x, const double* y, const double* amps, int32_t K);
/* the uploaded values: K (0: no table set) and, where asked for, K values each; amps and amps_slope are zeros without that column */
int brov_curve_get_table_host(brov_solver* s, int32_t which, double* x, double* y, double* slope, double* amps, double* amps_slope, int32_t* K);
/* switches the stage on with fresh books */
int brov_curve_set_host(brov_solver* s, const brov_curve_params* p, const double* eff /*[B][6]; NULL: 1*/);
int brov_curve_off(brov_solver* s);
int brov_curve_enabled(const brov_solver* s);   /* 0 for NULL */
int brov_curve_reset(brov_solver* s);           /* zeroes wanted, last_command, last_thrust, the applied records, the statistics and the step count */
/* the part(s) alone (BROV_CURVE_PART_*) with the configuration in force (before any brov_curve_set_host: the defaults): out [B][6] for
 * in [B][6], and amps_out [B][6] or NULL (zeros without an amps column in force or a THRUST part).  It moves nothing */
int brov_curve_eval_host(brov_solver* s, int32_t part, const double* in, double* out, double* amps_out);
/* what the last plant step was given and made of it; any may be NULL, not all */
int brov_curve_last_host(brov_solver* s, double* u0_applied /*[B][4]*/, double* wanted /*[B][6]*/, double* command /*[B][6]*/, double* thrust /*[B][6]*/);
int brov_curve_get_stats_host(brov_solver* s, double* err_sq /*[B]*/, int32_t* dead_ticks /*[B][6]*/, double* charge /*[B]*/, int64_t* steps);   /* any may be NULL */
int brov_curve_reset_stats(brov_solver* s);     /* err_sq, dead_ticks, charge and the step count to zero */
/* the last launch of either part, HIP events; one may be NULL.  A BOTH launch is both parts' last launch */
int brov_curve_last_seconds(brov_solver* s, double* command_s, double* thrust_s);

#endif
