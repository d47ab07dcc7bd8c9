// plant_stages.hpp -- the device side of the plant's stateless stages ahead of the model, shared by the plant kernels of plant_wrench.hip and
// plant_current.hip and plant_coriolis.hip: the world-frame wrench generator (brov_plant_wrench_*), the thruster stage with its accounting
// (brov_thruster_*) and the Coriolis stage's force (brov_coriolis_*), which model_f calls under its fourth tag.
// Written with explicitly rounded operations under `fp contract(off)` (hipcc otherwise contracts a product and a sum into an FMA, also across
// inlined calls), so that every kernel that inlines them and the numpy restatements of tests/ agree bit for bit.  Device code.
#pragma once
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"   // kMass, sincos_pio2, CoriolisStage
#include "rounded_ops.hpp"   // splitmix64_finalise, rn_mul, rn_add

namespace brov {

// the counter-based uniform draw in [0, 1) of instance b at index j (22 bits) in channel c (2 bits): 53 bits of one SplitMix64 output
__device__ __forceinline__ double counter_uniform(unsigned long long seed, int b, long long j, int c) {
#pragma clang fp contract(off)
    const unsigned long long n =((unsigned long long)b << 24) | ((unsigned long long)(j & 0x3FFFFF) << 2) | (unsigned long long)c;
    const unsigned long long z = splitmix64_finalise(seed + (n + 1ULL) * 0x9E3779B97F4A7C15ULL);
    return (double)(z >> 11) * 0x1.0p-53;   // exact: 53 bits
}

// amplitude of channel c (X = 0, Y = 1, Z = 2, N = 3) of instance b in half period j: scale * uniform[0.5, 1), counter-based
__device__ __forceinline__ double wrench_amplitude(const WrenchGen& g, int b, long long j, int c) {
#pragma clang fp contract(off)
    const double U = counter_uniform(g.seed, b, j, c);
    return __dmul_rn(g.scale, __dadd_rn(0.5, __dmul_rn(0.5, U)));
}

__device__ __forceinline__ void wrench_at(const WrenchGen& g, int b, long long k, double (&w)[6]) {
#pragma clang fp contract(off)
    if (g.mode == BROV_WRENCH_CONSTANT) {
#pragma unroll
        for (int c = 0; c < 6; c++) w[c] = g.w[(size_t)b * 6 + c];
    } else if (g.mode == BROV_WRENCH_TABLE) {
        long long r = k < 0 ? 0 : k;
        if (r > g.rows - 1) r = g.rows - 1;   // past the end: the last row, repeated (the reference indexes past the end)
        const double gn = g.gain ? g.gain[b] : 1.0;
#pragma unroll
        for (int c = 0; c < 6; c++) w[c] = __dmul_rn(g.tab[(size_t)r * 6 + c], gn);
    } else if (g.mode == BROV_WRENCH_PERIODIC) {
        const double t = __dadd_rn(g.phase0, __dmul_rn((double)k, g.dphi));   // a product, not the reference's running sum
        const long long j = (long long)floor(__ddiv_rn(t, 3.14159265358979323846));
        const double ax = wrench_amplitude(g, b, j, 0), ay = wrench_amplitude(g, b, j, 1), az = wrench_amplitude(g, b, j, 2);
        // (channel 3, the N amplitude, is drawn by the reference and never used: its counter value stays reserved)
        const double sn = sin(t);
        w[0] = __dmul_rn(sn, ax); w[1] = __dmul_rn(sn, ay); w[2] = __dmul_rn(sn, az);
        w[3] = 0.0; w[4] = 0.0;
        w[5] = __ddiv_rn(w[1], g.tz_div);   // the yaw torque follows the Y amplitude (:787)
    } else {
#pragma unroll
        for (int c = 0; c < 6; c++) w[c] = 0.0;
    }
}

// ---- the thruster stage (brov_thruster_*): limits, per-instance faults and the propulsion matrix between the six commands of the result
// record and the body wrench the model integrates.  For instance b at plant tick k, t = the commands:
//   c[i] = t[i] < lo[i] ? lo[i] : (t[i] > hi[i] ? hi[i] : t[i])                 (a NaN passes through)
//   a[i] = k >= onset[b] ? gain[b][i] * c[i] + bias[b][i] : c[i]                product rounded, then the sum
//   g[r] = ((((K[r][0] a[0] + K[r][1] a[1]) + K[r][2] a[2]) + K[r][3] a[3]) + K[r][4] a[4]) + K[r][5] a[5]
// every operation rounded on its own: the evaluation kernel, the plant kernels and the numpy restatement of tests/thruster_restatement.py
// agree bit for bit.  No state: any tick can be evaluated again.  (rn_mul / rn_add, and why not __dmul_rn / __dadd_rn: rounded_ops.hpp)
__device__ __forceinline__ void thruster_stage(const ThrusterPar& T, const ThrusterDev& D, int b, long long k, const double (&t)[6], double (&a)[6],
                                               double (&g)[6]) {
#pragma clang fp contract(off)
    const bool faulty = k >= D.onset[b];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double c = t[i] < T.lo[i] ? T.lo[i] : (t[i] > T.hi[i] ? T.hi[i] : t[i]);
        const double f = rn_add(rn_mul(D.gain[(size_t)b * 6 + i], c), D.bias[(size_t)b * 6 + i]);
        a[i] = faulty ? f : c;
    }
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double acc = rn_add(rn_mul(T.K[r * 6], a[0]), rn_mul(T.K[r * 6 + 1], a[1]));
#pragma unroll
        for (int i = 2; i < 6; i++) acc = rn_add(acc, rn_mul(T.K[r * 6 + i], a[i]));
        g[r] = acc;
    }
}

// what a plant step leaves behind per instance (one lane per instance, no atomics): ticks on which a command lay outside its limits, the
// running sum of |commanded - applied|^2 -- six squares summed in index order, then ONE add into the sum --, the thrusts applied
__device__ __forceinline__ void thruster_account(const ThrusterPar& T, const ThrusterDev& D, int b, const double (&t)[6], const double (&a)[6]) {
#pragma clang fp contract(off)
    double sq = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        D.clip_ticks[(size_t)b * 6 + i] += (t[i] < T.lo[i] || t[i] > T.hi[i]) ? 1 : 0;
        const double d = rn_add(t[i], -a[i]);
        sq = i == 0 ? rn_mul(d, d) : rn_add(sq, rn_mul(d, d));
        D.last[(size_t)b * 6 + i] = a[i];
    }
    D.lost_sq[b] = rn_add(D.lost_sq[b], sq);
}

// ---- the Coriolis stage (brov_coriolis_*): the Coriolis and centripetal forces of the vehicle the reference's observer is written for
// (BLUEROV2_DOB::f(), bluerov2_dob.cpp:651-677; dynamics_C(), :894-906), which the OCP model drops.  Rows X, Y, Z, N of -C_RB(nu) nu (m = kMass,
// CG at the origin) and of -C_A(nu_r) nu_r for the diagonal added mass (Xa, Ya, Za, ka, ma, .), at nu = (u v w p q r) and the velocity
// through the water nr = (ur vr wr):
//   RIGID:  cX = m ((r v) - (q w))      cY = m ((p w) - (r u))      cZ = m ((q u) - (p v))      cN = 0
//   ADDED:  ax = Xa ur, ay = Ya vr, az = Za wr;  bx = ka p, by = ma q
//           aX = (ay r) - (az q)        aY = (az p) - (ax r)        aZ = (ax q) - (ay p)        aN = ((ax vr) - (ay ur)) + ((bx q) - (by p))
//   both:   one add per channel, rigid + added
// every product and every difference rounded on its own, in the order written: coriolis_eval_kernel, model_f under its fourth tag and the
// numpy restatement of tests/coriolis_restatement.py agree bit for bit on the same inputs.  No state.  Both groups are computed and the
// terms SELECT among them: with a branch per group in each of the four inlined stages plant_coriolis_kernel needed 255 VGPRs and 48 AGPRs
// (occupancy 1); branch-free it needs 242 and none.
__device__ __forceinline__ void coriolis_force(const CoriolisStage& cs, const double (&nu)[6], const double (&nr)[3], double (&c)[4]) {
#pragma clang fp contract(off)
    const double u = nu[0], v = nu[1], w = nu[2], p = nu[3], q = nu[4], r = nu[5];
    const bool rigid = cs.terms & BROV_CORIOLIS_RIGID, added = cs.terms & BROV_CORIOLIS_ADDED;
    double g[4], a[4];
    g[0] = rn_mul(kMass, rn_add(rn_mul(r, v), -rn_mul(q, w)));
    g[1] = rn_mul(kMass, rn_add(rn_mul(p, w), -rn_mul(r, u)));
    g[2] = rn_mul(kMass, rn_add(rn_mul(q, u), -rn_mul(p, v)));
    g[3] = 0.0;
    const double ax = rn_mul(cs.xa, nr[0]), ay = rn_mul(cs.ya, nr[1]), az = rn_mul(cs.za, nr[2]);
    const double bx = rn_mul(cs.ka, p), by = rn_mul(cs.ma, q);
    a[0] = rn_add(rn_mul(ay, r), -rn_mul(az, q));
    a[1] = rn_add(rn_mul(az, p), -rn_mul(ax, r));
    a[2] = rn_add(rn_mul(ax, q), -rn_mul(ay, p));
    a[3] = rn_add(rn_add(rn_mul(ax, nr[1]), -rn_mul(ay, nr[0])), rn_add(rn_mul(bx, q), -rn_mul(by, p)));
#pragma unroll
    for (int i = 0; i < 4; i++) c[i] = (rigid && added) ? rn_add(g[i], a[i]) : (added ? a[i] : (rigid ? g[i] : 0.0));   // no terms: zeros
}

// the velocity through the water for coriolis_force where nothing but a state and a world-frame water velocity vc is at hand (the evaluation
// kernel, the `last` rows of the plant kernel): nr = x[6..9) - R^T vc with the attitude of x, R as model_f writes it from sincos_pio2, every
// product and sum rounded on its own, rows summed left to right.  (model_f's own projection is written for speed, with contractions.)
__device__ __forceinline__ void water_velocity(const double (&x)[NX], const double (&vc)[3], double (&nr)[3]) {
#pragma clang fp contract(off)
    double sph, cph, sth, cth, sps, cps;
    sincos_pio2(x[3], &sph, &cph);
    sincos_pio2(x[4], &sth, &cth);
    sincos_pio2(x[5], &sps, &cps);
    const double r00 = rn_mul(cps, cth), r01 = rn_add(rn_mul(rn_mul(cps, sth), sph), -rn_mul(sps, cph)),
                 r02 = rn_add(rn_mul(sps, sph), rn_mul(rn_mul(cps, cph), sth));
    const double r10 = rn_mul(sps, cth), r11 = rn_add(rn_mul(cps, cph), rn_mul(rn_mul(sph, sth), sps)),
                 r12 = rn_add(rn_mul(rn_mul(sth, sps), cph), -rn_mul(cps, sph));
    const double r20 = -sth, r21 = rn_mul(cth, sph), r22 = rn_mul(cth, cph);
    nr[0] = rn_add(x[6], -rn_add(rn_add(rn_mul(r00, vc[0]), rn_mul(r10, vc[1])), rn_mul(r20, vc[2])));
    nr[1] = rn_add(x[7], -rn_add(rn_add(rn_mul(r01, vc[0]), rn_mul(r11, vc[1])), rn_mul(r21, vc[2])));
    nr[2] = rn_add(x[8], -rn_add(rn_add(rn_mul(r02, vc[0]), rn_mul(r12, vc[1])), rn_mul(r22, vc[2])));
}

}  // namespace brov
