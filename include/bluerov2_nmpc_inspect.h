/* bluerov2_nmpc_inspect.h -- brov_range_* and brov_inspect_*: the bridge-pier inspection loop of the reference's third demo
 * (start_bridge_demo; bluerov2_dobmpc/src/bluerov2_inspection_node.cpp, the VisualController) on the device: a depth camera's mean range to
 * scene geometry, and the six-state mission machine with three PID loops that strafes along a pier at a stand-off distance, turns 90 degrees
 * at every edge and climbs after a round.  Part of the C ABI of bluerov2_nmpc.h, which includes this file behind bluerov2_nmpc_imu.h; not meant
 * to be included on its own.
 *
 * The range stage.  Scene: up to BROV_RANGE_MAX_BOXES axis-aligned WORLD-frame boxes {lo[3], hi[3]}, shared by the batch.  Camera: a square
 * region of interest of roi x roi pixels about the principal point of a pinhole camera with focal length f (pixels) whose optical axis is
 * body x.  Pixel (i, j), i, j = -roi/2 ... roi/2 - 1:  a = (i + 0.5 - cx) / f,  b = (j + 0.5 - cy) / f,  body-frame direction d = (1, -a, -b),
 * so the ray parameter t is the depth;  D = Rot(phi, theta, psi) d,  origin o = p + Rot mount.  Slab test per box and axis c:
 *   inv = 1 / D_c;  t1 = (lo_c - o_c) inv;  t2 = (hi_c - o_c) inv;  tn = fmax(tn, fmin(t1, t2));  tf = fmin(tf, fmax(t1, t2))   from -inf, +inf
 * with the NaN-ignoring IEEE fmin / fmax: the 0 * inf of a grazing ray is defined, and counts as a miss.  A box is hit iff tn <= tf,
 * tn >= near and tn <= far; the ray's depth is the smallest such tn over the boxes (none: no return), its range depth * sqrt(1 + a^2 + b^2).
 * Every product, sum and quotient is rounded once; a numpy restatement given the same Rot agrees per ray bit for bit
 * (tests/inspect_restatement.py).  One wavefront per instance: lane l takes the rays q = l, l + 64, ... (q = (j + roi/2) roi + (i + roi/2)) in
 * that order into a running sum and count, the 64 partials are combined in the fixed tree s[l] += s[l + stride], stride 32 ... 1, and
 *   range = sum / count, or 0.0 with count == 0 ("no pier in view": the reference's state machine reads it as pos.x < 0.1)
 * so the result depends neither on the batch nor on the launch.  With count > 0:  range + sigma[b] n(seed, b, m, 32), n the sensor stages'
 * counter-based variate at the free channel slot 32, m the plant's tick counter, which must stay in [0, 2^24).
 *
 * The controller.  One instance = one VisualController.  Inputs per tick: pos.x = the range (always from the TRUE state), pos.z = z,
 * pos.yaw = remainder(psi, 2 pi) (the exact IEEE operation) of the state the controller sees: the measured one while the sensor stage is on.
 * Time is k dt with the stage's own tick count k, which counts every tick since the reset.  Before a range > buffer was seen (`started`, the
 * node's is_start) the record is all zeros and only k moves.  The node's unqualified abs(double) is taken as fabs.  Its two quirks are flags,
 * both on by default:
 *   BROV_INSPECT_SHARED_PID   one integral and one previous error serve all three loops, in the call order of each branch (off: a pair per loop)
 *   BROV_INSPECT_FLOAT_YAW    yaw_sum, pre_yaw, yaw_diff and the goal height are single precision and round at every assignment
 * The controller writes the solver's own records (brov_results_device): status = BROV_STATUS_SUCCESS, cost = kkt = 0, qp_iter = 0,
 * u0 = (c1, c2, -c3, c4) -- the node publishes thrust4 = +c3 / rotor_constant where the MPC nodes publish -u0[2] / rotor_constant -- and
 * thrust = the solver's allocation of that u0, which is what the node publishes.  The delay, rotor and thruster stages, the logs and the
 * tracker work on them unchanged.
 * With the feature never set, and after brov_inspect_off, every launch is the one of a solver that never touched this API. */
#ifndef BLUEROV2_NMPC_INSPECT_H_
#define BLUEROV2_NMPC_INSPECT_H_
#ifndef BLUEROV2_NMPC_H_
#error "include bluerov2_nmpc.h, which includes this file"
#endif

#define BROV_RANGE_MAX_BOXES 8
typedef struct brov_range_params {
    double f;              /* focal length in pixels: > 0 (brov_range_focal) */
    double cx;             /* principal-point offset in pixels */
    double cy;
    double mount[3];       /* camera origin in the body frame */
    double near;           /* a return nearer than this is none */
    double far;            /* ... or farther than this: near < far */
    uint64_t seed;
    int32_t roi;           /* side of the region of interest in pixels: even, 2 ... 64 */
    int32_t reserved_;
} brov_range_params;
/* roi 40; f of the depth sensor that feeds /camera/depth/color/points (bluerov2_environ/urdf/_d435.gazebo.xacro: 1280 pixels over 85.2 degrees);
 * cx = cy = 0, mount 0, near 0.1, far 100, seed 0 */
void brov_range_default_params(brov_range_params* p);
double brov_range_focal(double width, double hfov);   /* width / (2 tan(hfov / 2)); pure host function */
/* the scene: n boxes, lo and hi [n][3].  Refused: n outside 0 ... BROV_RANGE_MAX_BOXES, a non-finite bound, lo > hi */
int brov_range_set_scene_host(brov_solver* s, int32_t n, const double* lo, const double* hi);
/* the camera and the noise.  Refused: roi odd or outside 2 ... 64, a non-finite parameter, f <= 0, near >= far, a negative or NaN sigma */
int brov_range_set_host(brov_solver* s, const brov_range_params* p, const double* sigma /*[B]; NULL: 0*/);
/* the stage alone at index m for the states x: the mean range (with the noise), the rays with a return, and optionally the rotation used and
 * the per-ray depths (0.0 where a ray has no return), row q as above.  It moves nothing */
int brov_range_eval_host(brov_solver* s, int64_t m, const double* x /*[B][12]*/, double* range /*[B]*/, int32_t* hits /*[B]*/,
                         double* rot /*[B][9] or NULL*/, double* depth /*[B][roi * roi] or NULL*/);
int brov_range_last_seconds(brov_solver* s, double* seconds);   /* the last launch that cast rays, HIP events */

#define BROV_INSPECT_SHARED_PID 1
#define BROV_INSPECT_FLOAT_YAW 2
typedef struct brov_inspect_params {
    double dt;             /* the controller's period: the plant steps of the loop must have exactly this dt */
    double safety_dis;     /* stand-off distance */
    double buffer;         /* half width of the stand-off band; a range above it starts the mission */
    double sway;           /* sway command along a face */
    double sway_slow;      /* ... near an edge */
    double surge_search;   /* surge command while looking for the next face */
    double z0;             /* initial depth reference */
    double yaw0;           /* initial yaw reference */
    double dz_round;       /* climb after a round: 2 safety_dis tan(32 deg), computed on the host */
    double lost;           /* a range below this is "no pier in view" */
    double yaw_tol;        /* a turn is complete within this of the yaw reference */
    double yaw_home_tol;   /* ... and the round when the yaw is within this of yaw0 */
    double z_tol;          /* the climb is complete within this of the depth reference */
    double height_tol;     /* the mission when the depth reference is within this of z_goal */
    double t_hold;         /* before this time: hold the start pose */
    double z_goal;         /* z0 + dz_round */
    double gains[9];       /* (kp, ki, kd) of the x, z and yaw loops */
    int32_t flags;         /* BROV_INSPECT_* */
    int32_t reserved_;
} brov_inspect_params;
void brov_inspect_default_params(brov_inspect_params* p);   /* the node's values; both flags */

typedef struct brov_inspect_state {
    double integral[3];    /* PID accumulators; BROV_INSPECT_SHARED_PID: [0] alone is used */
    double prev_error[3];
    double yaw_sum;        /* unwrapped yaw */
    double pre_yaw;
    double ref_x;
    double ref_z;
    double ref_yaw;
    int32_t started;
    int32_t turn;
    int32_t completed_turn;
    int32_t completed_round;
    int32_t get_height;
    int32_t completed_mission;
    int32_t cycle_counter;
    int32_t status;        /* 0 along a face, 1 near an edge, 2 turning, 3 searching, 4 climbing, 5 mission completed */
    int64_t k;             /* ticks of the stage since the reset */
} brov_inspect_state;
typedef struct brov_inspect_stats {
    int32_t ticks[6];      /* started ticks that ended in status 0 ... 5 */
    int32_t rounds;
    int32_t failed;        /* visits of the "state machine failed" branch */
    int32_t first_done;    /* first tick k with the mission completed, -1: none */
    int32_t reserved_;
    double standoff_sq;    /* sum of (range - safety_dis)^2 over the ticks that ended in status 0 */
    double min_range;      /* smallest non-zero range seen, 0: none */
} brov_inspect_stats;

/* The controller comes into force with a fresh state and statistics.  Refused with BROV_ERR_ARG and a text in brov_last_error() that starts
 * with the call's name, before anything touches a device: a non-finite parameter, dt <= 0, an unknown flag */
int brov_inspect_set_host(brov_solver* s, const brov_inspect_params* p);
int brov_inspect_off(brov_solver* s);
int brov_inspect_enabled(const brov_solver* s);   /* 0 for NULL */
int brov_inspect_reset(brov_solver* s);           /* the initial state of the node's constructor, k = 0; the statistics stay */
/* the controller alone with the parameters in force (before any brov_inspect_set_host: the defaults): one tick from state_in on the given
 * range, z and psi.  stats: in and out, NULL: none.  It moves nothing */
int brov_inspect_eval_host(brov_solver* s, const brov_inspect_state* state_in /*[B]*/, const double* range /*[B]*/, const double* z /*[B]*/,
                           const double* psi /*[B]*/, brov_inspect_state* state_out /*[B]*/, brov_result* rec /*[B]*/,
                           brov_inspect_stats* stats /*[B] or NULL*/);
int brov_inspect_get_state_host(brov_solver* s, brov_inspect_state* state /*[B]*/, double* range /*[B] the last range, or NULL*/);
int brov_inspect_get_stats_host(brov_solver* s, brov_inspect_stats* stats /*[B]*/);
int brov_inspect_reset_stats(brov_solver* s);
int brov_inspect_last_seconds(brov_solver* s, double* seconds);   /* the tick kernel's last launch, HIP events */
/* One tick: one launch (inspect_tick_kernel, one wavefront per instance).  The lanes cast the rays from the TRUE state at the plant's tick
 * counter; lane 0 then runs the controller on the state the controller sees and writes the record, the state, the statistics, the last range
 * and the status.  Refused: the controller off, no box in the scene, an index outside [0, 2^24) */
int brov_inspect_step(brov_solver* s, void* stream);
/* The loop as one call: per tick brov_inspect_step -> brov_plant_step(s, dt, substeps) with every stage that is on, on the solver's last
 * stream, one host wait at the end.  Logs (HOST, any NULL): u_log [ticks][B][4], x_log [ticks + 1][B][12], st_log [ticks][B] the mission
 * status, r_log [ticks][B] the range.  They are bit for bit those of the same calls composed by the caller.  Refused: what brov_inspect_step
 * refuses, a dt that is not bit-equal to the controller's (the rotor stage's rule), a delay stage with comp > 0 (there is no solve to
 * predict for), and what the stages in force refuse of those plant steps */
int brov_closed_loop_inspect(brov_solver* s, int ticks, double dt, int substeps, double* u_log, double* x_log, int32_t* st_log, double* r_log);

#endif
