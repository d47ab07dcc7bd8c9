// bluerov2_model.hpp -- device-side BlueROV2 model for gfx950 (FP64).
//
// Hand-derived f(x,u,p) and the action of its Jacobian on a direction (A_c s), exploiting the 48/144 sparsity of
// df/dx, the constancy of df/du and the rotation-matrix structure of the kinematic rows.  Follows the OCP definition
// /root/reference/bluerov2_dobmpc/scripts/bluerov2.py:77-137 (incl. the sin(psi) term of dphi, :133) and the
// derivative conventions of the generated c_generated_code/bluerov2_model/bluerov2_expl_vde_forw.c
// (d|v|v/dv = sign(v) v + |v| = 2|v|, zero at v = 0, :65).  Not a translation of the CasADi code: no common file
// structure, ~130 flops per Jacobian-vector product instead of a 4.5k-statement dense VDE.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace brov {

constexpr int NX = 12, NU = 4, NP = 16, NY = 16;

// bluerov2.py:77-84
constexpr double kMass = 11.26, kIx = 0.3, kIy = 0.63, kIz = 0.58, kZG = 0.02, kG = 9.81, kBouy = 0.66;
constexpr double kRotor = 0.026546960744430276;
constexpr double kMzg = kMass * kZG * kG;

// parameter-derived constants of one stage (p = [dist4 | added mass4 | linear damping4 | quadratic damping4])
struct ModelPar {
    double dx, dy, dz, dn;      // disturbances
    double imx, imy, imz, imn;  // 1/(m+Xa), 1/(m+Ya), 1/(m+Za), 1/(Iz+Na)
    double lx, ly, lz, ln;      // linear damping
    double qx, qy, qz, qn;      // quadratic damping
};

// 1/d for a positive, normal d: v_rcp_f64 seed + 2 Newton steps (~1 ulp) -- an IEEE division is ~35 dependent instructions
__device__ __forceinline__ double rcp_nr(double d) {
    double y = __builtin_amdgcn_rcp(d);
    double e = fma(-d, y, 1.0);
    y = fma(y, e, y);
    e = fma(-d, y, 1.0);
    return fma(y, e, y);
}

__device__ __forceinline__ ModelPar make_par(const double* __restrict__ p) {
    ModelPar m;
    m.dx = p[0]; m.dy = p[1]; m.dz = p[2]; m.dn = p[3];
    m.imx = rcp_nr(kMass + p[4]); m.imy = rcp_nr(kMass + p[5]); m.imz = rcp_nr(kMass + p[6]);
    m.imn = rcp_nr(kIz + p[7]);
    m.lx = p[8]; m.ly = p[9]; m.lz = p[10]; m.ln = p[11];
    m.qx = p[12]; m.qy = p[13]; m.qz = p[14]; m.qn = p[15];
    return m;
}

// generalised forces of the 6 thrusters for the 4 wrench commands (bluerov2.py:95-121), constant over an RK step
// k3 / k4: roll / pitch moments.  The propulsion matrix gives the thrusters none (K rows 3, 4 are zero, bluerov2.py:95-100); they carry
// the roll / pitch DISTURBANCE moments of the 6-disturbance model variant (the symbols bluerov2.py:37-38 keeps commented out,
// entering dp, dq the way the other four disturbances enter their rows, :123-128) and are 0 in the shipped np = 16 model.
struct Wrench { double k0, k1, k2, k5, k3, k4; };

__device__ __forceinline__ Wrench make_wrench(const double* __restrict__ u) {
    const double ir = 1.0 / kRotor;
    const double t0 = (-u[0] + u[1] + u[3]) * ir, t1 = (-u[0] - u[1] - u[3]) * ir;
    const double t2 = (u[0] + u[1] - u[3]) * ir, t3 = (u[0] - u[1] + u[3]) * ir;
    const double t4 = -u[2] * ir;
    Wrench w;
    w.k0 = 0.707 * t0 + 0.707 * t1 - 0.707 * t2 - 0.707 * t3;
    w.k1 = 0.707 * t0 - 0.707 * t1 + 0.707 * t2 - 0.707 * t3;
    w.k2 = t4 + t4;
    w.k5 = 0.167 * t0 - 0.167 * t1 - 0.175 * t2 + 0.175 * t3;
    w.k3 = 0.0; w.k4 = 0.0;
    return w;
}

// sin and cos together, branch-free: 3-term Cody-Waite reduction by pi/2 (FMA) + the classic degree-13/14 minimax kernels
// on [-pi/4, pi/4].  Measured for |a| <= 1e6 rad (yaw_sum of the reference grows by 2 pi per lap, i.e. a few hundred rad at most): at most
// 1.53 ulp (sin, at a = -547.42; cos 1.45), no quadrant error, also at the doubles next to k pi/2 (profiles/model_exact.txt; held to 2 ulp
// by tests/test_gpu_model_exact.py); sin(-0.0) = +0; NaN/Inf give NaN.  ocml's sincos() costs ~3x the registers and pushed the linearisation kernel into scratch.
__device__ __forceinline__ void sincos_pio2(double a, double* sn, double* cs) {
    const double n = rint(a * 6.36619772367581382433e-01);
    double r = fma(-n, 1.57079632679489655800e+00, a);
    r = fma(-n, 6.12323399573676603587e-17, r);
    r = fma(-n, -1.49738490485916983e-33, r);
    const double z = r * r;
    double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    ps = fma(z, ps, 2.75573137070700676789e-06);
    ps = fma(z, ps, -1.98412698298579493134e-04);
    ps = fma(z, ps, 8.33333333332248946124e-03);
    ps = fma(z, ps, -1.66666666666666324348e-01);
    const double s = fma(r * z, ps, r);
    double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    pc = fma(z, pc, -2.75573143513906633035e-07);
    pc = fma(z, pc, 2.48015872894767294178e-05);
    pc = fma(z, pc, -1.38888888888741095749e-03);
    pc = fma(z, pc, 4.16666666666666019037e-02);
    const double c = fma(z * z, pc, fma(z, -0.5, 1.0));
    const int q = (int)n & 3;
    const double s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
    *sn = (q & 2) ? -s1 : s1;
    *cs = ((q + 1) & 2) ? -c1 : c1;
}

// what one RK stage point contributes to the Jacobian: 6 trig values, 1/cos(theta), body velocities and rates
struct StagePoint {
    double sph, cph, sth, cth, sps, cps, icth;
    double vu, vv, vw, wp, wq, wr;
};

// A wrench given in the WORLD frame (the reference's applyBodyWrench(), bluerov2_dob.cpp:876-890: reference_frame = "world"), constant
// over a control tick; its body-frame image turns with the vehicle.  NoWorldWrench: the tag of a model without one.
struct WorldWrench { double fx, fy, fz, tx, ty, tz; };
struct NoWorldWrench {};
// A world wrench (possibly zero) AND an ocean current: a WORLD-frame water velocity (vx, vy, vz) in m/s, constant over a control tick (the
// reference's underwater_current_plugin, bluerov2_environ/worlds/ocean_waves.world).  The third tag of model_f: the plant of plant_current.hip.
struct WorldWrenchCurrent { WorldWrench ww; double vx, vy, vz; };
// ... AND the Coriolis and centripetal forces the OCP model drops (brov_coriolis_*): the fourth tag of model_f, the plant of plant_coriolis.hip.
// terms: BROV_CORIOLIS_* bit mask; xa, ya, za: the instance's true added masses p[4..6]; ka, ma: the stage's roll / pitch added inertia.
struct CoriolisStage { int terms; double xa, ya, za, ka, ma; };
struct WorldWrenchCurrentCoriolis { WorldWrenchCurrent wc; CoriolisStage cs; };
// c = [X Y Z N], the stage's force at the body velocities nu = (u v w p q r) and the velocity through the water nr: plant_stages.hpp, which a
// file that instantiates the fourth tag includes
__device__ __forceinline__ void coriolis_force(const CoriolisStage& cs, const double (&nu)[6], const double (&nr)[3], double (&c)[4]);
// the wrench-and-current part of either tag that has one
__device__ __forceinline__ const WorldWrenchCurrent& current_part(const WorldWrenchCurrent& w) { return w; }
__device__ __forceinline__ const WorldWrenchCurrent& current_part(const WorldWrenchCurrentCoriolis& w) { return w.wc; }

// xdot = f(x,u,p), WW = NoWorldWrench: the model of the OCP; also returns the stage point record.
// WW = WorldWrench: the same model under an additional world-frame wrench, the plant of brov_plant_step with a wrench mode in force
// (plant_wrench.hip).  Force and torque are projected with THIS stage point's attitude, f_b = R^T f_w, t_b = R^T t_w -- from the trig
// values the model computes anyway -- and enter where the model's own disturbances do: dx, dy, dz, k3, k4, dn, ahead of the mass scaling.
// One body for both: the projection sits under `if constexpr`, so the NoWorldWrench instantiation holds no statement of it and the
// solver kernels that inline it -- at their register limit, behind the build's scratch gate and ISA checkers -- compile to the code they
// compiled to when the function had no such parameter (profiles/plant_step_refactor_isa.txt: instruction for instruction).
// WW = WorldWrenchCurrent: the world wrench as above, and the water moves: the current is projected like the force, c = R^T vc, and the two
// damping terms of rows 6, 7, 8 are evaluated at the velocity through the water, v - c.  Quasi-static drag only: the state stays the velocity
// over ground, and no other row sees the current (profiles/current_isa.txt: the other two instantiations unchanged).
// WW = WorldWrenchCurrentCoriolis: the third tag, and the rigid-body and added-mass Coriolis forces of rows X, Y, Z, N (coriolis_force,
// plant_stages.hpp) at this stage point's velocities -- the added-mass group at the velocity through the water -- enter where the model's own
// disturbances do: dx, dy, dz, dn (profiles/coriolis_isa.txt: the other three instantiations unchanged).
template <class WW>
__device__ __forceinline__ void model_f(const double (&x)[NX], const Wrench& w, const ModelPar& m, const WW& ww, double (&f)[NX],
                                        StagePoint& sp) {
    static_assert(std::is_same_v<WW, WorldWrench> || std::is_same_v<WW, NoWorldWrench> || std::is_same_v<WW, WorldWrenchCurrent> ||
                      std::is_same_v<WW, WorldWrenchCurrentCoriolis>,
                  "a world wrench, a world wrench with a current, the two under the Coriolis stage, or the tag for none");
    sincos_pio2(x[3], &sp.sph, &sp.cph);
    sincos_pio2(x[4], &sp.sth, &sp.cth);
    sincos_pio2(x[5], &sp.sps, &sp.cps);
    sp.icth = 1.0 / sp.cth;
    sp.vu = x[6]; sp.vv = x[7]; sp.vw = x[8]; sp.wp = x[9]; sp.wq = x[10]; sp.wr = x[11];
    const double r00 = sp.cps * sp.cth, r01 = sp.cps * sp.sth * sp.sph - sp.sps * sp.cph,
                 r02 = sp.sps * sp.sph + sp.cps * sp.cph * sp.sth;
    const double r10 = sp.sps * sp.cth, r11 = sp.cps * sp.cph + sp.sph * sp.sth * sp.sps,
                 r12 = sp.sth * sp.sps * sp.cph - sp.cps * sp.sph;
    const double r20 = -sp.sth, r21 = sp.cth * sp.sph, r22 = sp.cth * sp.cph;
    double dx = m.dx, dy = m.dy, dz = m.dz, k3 = w.k3, k4 = w.k4, dn = m.dn;
    if constexpr (std::is_same_v<WW, WorldWrench>) {
        dx += (r00 * ww.fx + r10 * ww.fy + r20 * ww.fz);
        dy += (r01 * ww.fx + r11 * ww.fy + r21 * ww.fz);
        dz += (r02 * ww.fx + r12 * ww.fy + r22 * ww.fz);
        k3 += (r00 * ww.tx + r10 * ww.ty + r20 * ww.tz);
        k4 += (r01 * ww.tx + r11 * ww.ty + r21 * ww.tz);
        dn += (r02 * ww.tx + r12 * ww.ty + r22 * ww.tz);
    }
    double ur = sp.vu, vr = sp.vv, wr = sp.vw;   // velocity through the water: over ground, unless there is a current
    if constexpr (std::is_same_v<WW, WorldWrenchCurrent> || std::is_same_v<WW, WorldWrenchCurrentCoriolis>) {
        const WorldWrenchCurrent& wc = current_part(ww);
        dx += (r00 * wc.ww.fx + r10 * wc.ww.fy + r20 * wc.ww.fz);
        dy += (r01 * wc.ww.fx + r11 * wc.ww.fy + r21 * wc.ww.fz);
        dz += (r02 * wc.ww.fx + r12 * wc.ww.fy + r22 * wc.ww.fz);
        k3 += (r00 * wc.ww.tx + r10 * wc.ww.ty + r20 * wc.ww.tz);
        k4 += (r01 * wc.ww.tx + r11 * wc.ww.ty + r21 * wc.ww.tz);
        dn += (r02 * wc.ww.tx + r12 * wc.ww.ty + r22 * wc.ww.tz);
        ur -= (r00 * wc.vx + r10 * wc.vy + r20 * wc.vz);
        vr -= (r01 * wc.vx + r11 * wc.vy + r21 * wc.vz);
        wr -= (r02 * wc.vx + r12 * wc.vy + r22 * wc.vz);
    }
    if constexpr (std::is_same_v<WW, WorldWrenchCurrentCoriolis>) {
        const double nu[6] = {sp.vu, sp.vv, sp.vw, sp.wp, sp.wq, sp.wr}, nr[3] = {ur, vr, wr};
        double c[4];
        coriolis_force(ww.cs, nu, nr, c);   // evaluated afresh at every stage
        dx += c[0]; dy += c[1]; dz += c[2]; dn += c[3];
    }
    f[0] = r00 * sp.vu + r01 * sp.vv + r02 * sp.vw;
    f[1] = r10 * sp.vu + r11 * sp.vv + r12 * sp.vw;
    f[2] = r20 * sp.vu + r21 * sp.vv + r22 * sp.vw;   // (r20 * vu is the product -sth * vu: the unary minus binds first)
    const double tth = sp.sth * sp.icth;
    f[3] = sp.wp + sp.sps * tth * sp.wq + sp.cph * tth * sp.wr;  // sin(psi): reference quirk, bluerov2.py:133
    f[4] = sp.cph * sp.wq + sp.sph * sp.wr;
    f[5] = (sp.sph * sp.wq + sp.cph * sp.wr) * sp.icth;
    f[6] = (w.k0 - kBouy * sp.sth + dx + m.lx * ur + m.qx * fabs(ur) * ur) * m.imx;
    f[7] = (w.k1 + kBouy * r21 + dy + m.ly * vr + m.qy * fabs(vr) * vr) * m.imy;
    f[8] = (w.k2 + kBouy * r22 + dz + m.lz * wr + m.qz * fabs(wr) * wr) * m.imz;
    f[9] = (k3 + (kIy - kIz) * sp.wq * sp.wr - kMzg * r21) * (1.0 / kIx);
    f[10] = (k4 + (kIz - kIx) * sp.wp * sp.wr - kMzg * sp.sth) * (1.0 / kIy);
    f[11] = (w.k5 - (kIy - kIx) * sp.wp * sp.wq + dn + m.ln * sp.wr + m.qn * fabs(sp.wr) * sp.wr) * m.imn;
}

// ---- the one plant step of the device ------------------------------------------------------------------------------------------------
// One explicit RK4 step of size h (gen/acados_solver_bluerov2.c:633-641: 4 stages), xn = x+; sp[i] = the stage point of stage i, which
// the linearisation keeps (lin_device.hpp, rk4_state) and the plants below let die.
template <class WW>
__device__ __forceinline__ void erk4_step(const double (&x)[NX], const Wrench& w, const ModelPar& m, const WW& ww, double h,
                                          StagePoint (&sp)[4], double (&xn)[NX]) {
    double k[NX], xs[NX];
    model_f(x, w, m, ww, k, sp[0]);
#pragma unroll
    for (int j = 0; j < NX; j++) { xn[j] = x[j] + (h / 6.0) * k[j]; xs[j] = x[j] + 0.5 * h * k[j]; }
    model_f(xs, w, m, ww, k, sp[1]);
#pragma unroll
    for (int j = 0; j < NX; j++) { xn[j] += (h / 3.0) * k[j]; xs[j] = x[j] + 0.5 * h * k[j]; }
    model_f(xs, w, m, ww, k, sp[2]);
#pragma unroll
    for (int j = 0; j < NX; j++) { xn[j] += (h / 3.0) * k[j]; xs[j] = x[j] + h * k[j]; }
    model_f(xs, w, m, ww, k, sp[3]);
#pragma unroll
    for (int j = 0; j < NX; j++) xn[j] += (h / 6.0) * k[j];
}

// x <- the state one control period dt later, in `substeps` ERK4 steps with input and wrenches held.  The plant of plant_kernel
// and plant_thruster_kernel (plant_wrench.hip), plant_current_kernel (plant_current.hip), plant_coriolis_kernel (plant_coriolis.hip) and fleet_plant_kernel (fleet_kernel.hip).  NOT of plant_wrench_kernel (plant_wrench.hip) and plant_step_wave
// (qp/fused.hpp), which restate erk4_step's statements for the reasons given there: a change to the step is made here AND in those two.
template <class WW>
__device__ __forceinline__ void plant_erk4(double (&x)[NX], const Wrench& w, const ModelPar& m, const WW& ww, double dt, int substeps) {
    const double h = dt / substeps;
    StagePoint sp[4];
    double xn[NX];
    for (int s = 0; s < substeps; s++) {
        erk4_step(x, w, m, ww, h, sp, xn);
#pragma unroll
        for (int j = 0; j < NX; j++) x[j] = xn[j];
    }
}

// what a plant step of one instance starts from: x, u = its state and input, p = its 16 true parameters; 6-disturbance variant: its two
// roll / pitch disturbance moments at rp[rp_off], rp[rp_off + 1] (rp = nullptr: the shipped model, none)
__device__ __forceinline__ void plant_inputs(const double* x0, const double* u0, const double* p, const double* rp,
                                             size_t rp_off, double (&x)[NX], double (&u)[NU], ModelPar& m, Wrench& w) {
#pragma unroll
    for (int j = 0; j < NX; j++) x[j] = x0[j];
#pragma unroll
    for (int j = 0; j < NU; j++) u[j] = u0[j];
    m = make_par(p);
    w = make_wrench(u);
    if (rp) { w.k3 = rp[rp_off]; w.k4 = rp[rp_off + 1]; }
}

// dst[0 .. n) = v
template <int n>
__device__ __forceinline__ void store_row(double* dst, const double (&v)[n]) {
#pragma unroll
    for (int j = 0; j < n; j++) dst[j] = v[j];
}
// row `row` of a log of n doubles per row, if the log is kept (log = nullptr: it is not)
template <int n>
__device__ __forceinline__ void log_row(double* log, size_t row, const double (&v)[n]) {
    if (log) store_row(log + row * n, v);
}

}  // namespace brov
