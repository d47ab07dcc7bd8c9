// range_device.hpp -- what the kernels of the inspection loop share (inspect_kernel.hip: the box scene; mesh_kernel.hip: boxes and a triangle
// mesh): the rotation, the rays of a wavefront with the box loop and the tree sum, the mesh traversal with the ray-triangle test
// (include/bluerov2_nmpc_mesh.h has its formulas), and the controller.  One body each, so the two files cannot drift apart; the box-only
// instantiation holds no trace of the mesh.  Every operation is rounded on its own: the including file switches fp contract off, the sums and
// products the restatements restate bit for bit are written with rn_add / rn_mul, the quotients are IEEE divisions, the square root is
// __dsqrt_rn.  Device code.
#pragma once
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "mesh_device.hpp"
#include "bluerov2_model.hpp"   // sincos_pio2, kRotor
#include "rounded_ops.hpp"

#pragma clang fp contract(off)

namespace brov {

constexpr int kRangeSlot = 32;   // the noise channel of the range: the sensor stage draws at 0..12, the IMU/GPS stage at 16..28
constexpr double kTwoPi = 6.283185307179586, kHalfPi = 1.5707963267948966;

// the rotation of the model body (bluerov2_model.hpp: model_f's r00 ... r22), every operation rounded on its own
__device__ __forceinline__ void range_rot(double phi, double theta, double psi, double (&R)[9]) {
    double sph, cph, sth, cth, sps, cps;
    sincos_pio2(phi, &sph, &cph);
    sincos_pio2(theta, &sth, &cth);
    sincos_pio2(psi, &sps, &cps);
    R[0] = rn_mul(cps, cth); R[1] = rn_add(rn_mul(rn_mul(cps, sth), sph), -rn_mul(sps, cph)); R[2] = rn_add(rn_mul(sps, sph), rn_mul(rn_mul(cps, cph), sth));
    R[3] = rn_mul(sps, cth); R[4] = rn_add(rn_mul(cps, cph), rn_mul(rn_mul(sph, sth), sps)); R[5] = rn_add(rn_mul(rn_mul(sth, sps), cph), -rn_mul(cps, sph));
    R[6] = -sth;             R[7] = rn_mul(cth, sph);                                         R[8] = rn_mul(cth, cph);
}

// cross and dot products of the ray-triangle test: rn(rn(a b) - rn(c d)) per component, the dot product summed left to right
__device__ __forceinline__ void mesh_cross(const double (&a)[3], const double (&b)[3], double (&r)[3]) {
    r[0] = rn_add(rn_mul(a[1], b[2]), -rn_mul(a[2], b[1]));
    r[1] = rn_add(rn_mul(a[2], b[0]), -rn_mul(a[0], b[2]));
    r[2] = rn_add(rn_mul(a[0], b[1]), -rn_mul(a[1], b[0]));
}
__device__ __forceinline__ double mesh_dot(const double (&a)[3], const double (&b)[3]) {
    return rn_add(rn_add(rn_mul(a[0], b[0]), rn_mul(a[1], b[1])), rn_mul(a[2], b[2]));
}

// one ray (o, D, inv = 1 / D per component) through the mesh: the smallest hit t below `best` replaces it.  A forward walk over the nodes in
// depth-first order: a node is culled when its slabs do not overlap, end ahead of near or begin behind min(best, far); a culled node and a
// leaf go on at their skip link, an interior node at the next index.  nt, tt: node tests and triangle tests made
__device__ __forceinline__ void mesh_ray(const MeshDev& M, double near, double far, const double (&o)[3], const double (&D)[3], const double (&inv)[3],
                                         double& best, int& nt, int& tt) {
    const double inf = __builtin_huge_val();
    int i = 0;
    while (i < M.n_nodes) {
        const MeshNode* __restrict__ nd = M.nodes + i;
        double tn = -inf, tf = inf;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double t1 = rn_mul(rn_add(nd->lo[c], -o[c]), inv[c]), t2 = rn_mul(rn_add(nd->hi[c], -o[c]), inv[c]);
            tn = fmax(tn, fmin(t1, t2));
            tf = fmin(tf, fmax(t1, t2));
        }
        const int skip = nd->skip, first = nd->first, count = nd->count;
        nt++;
        if (!(tn <= tf) || tf < near || tn > fmin(best, far)) { i = skip; continue; }
        for (int k = first; k < first + count; k++) {
            const MeshTri* __restrict__ T = M.tris + k;
            double v0[3], e1[3], e2[3], p[3], s[3], q[3];
#pragma unroll
            for (int c = 0; c < 3; c++) { v0[c] = T->v0[c]; e1[c] = T->e1[c]; e2[c] = T->e2[c]; }
            mesh_cross(D, e2, p);
            const double det = mesh_dot(e1, p), idet = 1.0 / det;
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] = rn_add(o[c], -v0[c]);
            const double u = rn_mul(mesh_dot(s, p), idet);
            mesh_cross(s, e1, q);
            const double v = rn_mul(mesh_dot(D, q), idet), t = rn_mul(mesh_dot(e2, q), idet);
            tt++;
            if (det != 0.0 && u >= 0.0 && v >= 0.0 && rn_add(u, v) <= 1.0 && t >= near && t <= far && t < best) best = t;
        }
        i = count > 0 ? skip : i + 1;
    }
}

// the rays of instance b (wave-uniform) from the state x: the mean range with its noise and the number of returns, valid in lane 0.  MESH:
// the rays meet the triangles of M as well as the boxes of S; visits (lane 0, or nullptr): [2] node tests and triangle tests of the instance
template <bool MESH>
__device__ __forceinline__ void range_wave_on(const brov_range_params& P, const RangeScene& S, const MeshDev& M, const double* __restrict__ sigma, int b, int m,
                                              int lane, const double* __restrict__ x, double* __restrict__ rot, double* __restrict__ depth,
                                              double& range_out, int& hits_out, long long* __restrict__ visits) {
    double R[9], o[3];
    range_rot(x[3], x[4], x[5], R);
#pragma unroll
    for (int c = 0; c < 3; c++)
        o[c] = rn_add(x[c], rn_add(rn_add(rn_mul(R[c * 3], P.mount[0]), rn_mul(R[c * 3 + 1], P.mount[1])), rn_mul(R[c * 3 + 2], P.mount[2])));
    if (rot && lane < 9) {
        double r = R[0];
#pragma unroll
        for (int k = 1; k < 9; k++) r = lane == k ? R[k] : r;
        rot[(size_t)b * 9 + lane] = r;
    }
    const int roi = P.roi, half = roi >> 1, rays = roi * roi, nbox = S.n;
    const double inf = __builtin_huge_val();
    double sum = 0.0;
    int count = 0, nt = 0, tt = 0;
    for (int q = lane; q < rays; q += 64) {
        const int j = q / roi, i = q - j * roi;
        const double a = rn_add((double)(i - half) + 0.5, -P.cx) / P.f, bb = rn_add((double)(j - half) + 0.5, -P.cy) / P.f;
        double D[3], inv[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            D[c] = rn_add(rn_add(R[c * 3], rn_mul(R[c * 3 + 1], -a)), rn_mul(R[c * 3 + 2], -bb));
            inv[c] = 1.0 / D[c];
        }
        double best = inf;
        for (int k = 0; k < nbox; k++) {
            double tn = -inf, tf = inf;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double t1 = rn_mul(rn_add(S.lo[k][c], -o[c]), inv[c]), t2 = rn_mul(rn_add(S.hi[k][c], -o[c]), inv[c]);
                tn = fmax(tn, fmin(t1, t2));
                tf = fmin(tf, fmax(t1, t2));
            }
            if (tn <= tf && tn >= P.near && tn <= P.far && tn < best) best = tn;
        }
        if constexpr (MESH) mesh_ray(M, P.near, P.far, o, D, inv, best, nt, tt);
        const bool hit = best < inf;
        if (hit) {
            sum = rn_add(sum, rn_mul(best, __dsqrt_rn(rn_add(rn_add(1.0, rn_mul(a, a)), rn_mul(bb, bb)))));
            count++;
        }
        if (depth) depth[(size_t)b * rays + q] = hit ? best : 0.0;
    }
    // the fixed tree s[l] += s[l + stride]: lane l < stride reads lane l + stride; what the lanes above it hold is never read again
#pragma unroll
    for (int stride = 32; stride >= 1; stride >>= 1) {
        sum = rn_add(sum, __shfl_down(sum, stride, 64));
        count += __shfl_down(count, stride, 64);
    }
    if constexpr (MESH) {
        if (visits) {   // (wave-uniform; a lane's counts fit an int: 64 rays x 2^21 nodes)
            long long n = nt, t = tt;
#pragma unroll
            for (int stride = 32; stride >= 1; stride >>= 1) {
                n += __shfl_down(n, stride, 64);
                t += __shfl_down(t, stride, 64);
            }
            if (lane == 0) { visits[0] = n; visits[1] = t; }
        }
    }
    double range = 0.0;
    if (count > 0) {
        range = sum / (double)count;
        range = rn_add(range, rn_mul(sigma[b], sensor_noise(P.seed, b, m, kRangeSlot)));
    }
    range_out = range;
    hits_out = count;
}

// ---- the controller ------------------------------------------------------------------------------------------------------------------
struct InspectPid {
    const brov_inspect_params& C;
    brov_inspect_state& s;
    // the node's PID(): loop 0 x, 1 z, 2 yaw
    __device__ __forceinline__ double operator()(int loop, double ref, double pos) const {
        const bool sh = (C.flags & BROV_INSPECT_SHARED_PID) != 0;   // (static indices only: the state stays in registers)
        double I = sh ? s.integral[0] : s.integral[loop];
        const double pe = sh ? s.prev_error[0] : s.prev_error[loop];
        const double e = rn_add(ref, -pos);
        I = rn_add(I, rn_mul(e, C.dt));
        const double d = rn_add(e, -pe) / C.dt;
        const double out = rn_add(rn_add(rn_mul(C.gains[loop * 3], e), rn_mul(C.gains[loop * 3 + 1], I)), rn_mul(C.gains[loop * 3 + 2], d));
        if (sh) { s.integral[0] = I; s.prev_error[0] = e; } else { s.integral[loop] = I; s.prev_error[loop] = e; }
        return out;
    }
};

// one tick of instance's controller: state s and, with `stats`, statistics t move, the record is written whole
__device__ __forceinline__ void inspect_control(const brov_inspect_params& C, brov_inspect_state& s, brov_inspect_stats& t, bool stats, double range, double z,
                                                double psi, brov_result& rec) {
    const long long k = s.k;
    s.k = k + 1;
    if (stats && range != 0.0 && (t.min_range == 0.0 || range < t.min_range)) t.min_range = range;
    if (range > C.buffer) s.started = 1;
    double c1 = 0.0, c2 = 0.0, c3 = 0.0, c4 = 0.0;
    if (s.started) {
        const bool fl = (C.flags & BROV_INSPECT_FLOAT_YAW) != 0;
        auto F = [fl](double v) { return fl ? (double)(float)v : v; };
        const double yaw = remainder(psi, kTwoPi), pre = s.pre_yaw;
        double diff;
        if (pre >= 0.0 && yaw >= 0.0) diff = F(rn_add(yaw, -pre));
        else if (pre >= 0.0 && yaw < 0.0) {
            const double wrap = rn_add(rn_add(kTwoPi, yaw), -pre), direct = rn_add(pre, fabs(yaw));
            diff = wrap >= direct ? F(-direct) : F(wrap);
        } else if (pre < 0.0 && yaw >= 0.0) {
            const double wrap = rn_add(rn_add(kTwoPi, -yaw), pre), direct = rn_add(fabs(pre), yaw);
            diff = wrap >= direct ? F(direct) : F(-wrap);
        } else diff = F(rn_add(yaw, -pre));
        s.yaw_sum = F(rn_add(s.yaw_sum, diff));
        s.pre_yaw = F(yaw);

        const InspectPid pid{C, s};
        const double band_lo = rn_add(C.safety_dis, -C.buffer), band_hi = rn_add(C.safety_dis, C.buffer);
        const bool in_band = range >= band_lo && range <= band_hi;
        bool failed = false;
        if (rn_mul((double)k, C.dt) < C.t_hold) {
            c1 = pid(0, C.safety_dis, range);
            c3 = pid(1, C.z0, z);
            c4 = pid(2, C.yaw0, s.yaw_sum);
        } else if (!s.completed_mission) {
            if (in_band && s.completed_turn && !s.completed_round) {   // along a face: keep the stand-off, strafe
                s.status = 0;
                s.ref_x = C.safety_dis;
                c1 = pid(0, s.ref_x, range);
                c3 = pid(1, s.ref_z, z);
                c4 = pid(2, s.ref_yaw, s.yaw_sum);
                c2 = C.sway;
                s.completed_turn = 1; s.turn = 0; s.get_height = 1;
            } else if (range > band_hi && s.completed_turn) {          // near an edge: no surge control, strafe slowly
                s.status = 1;
                c3 = pid(1, s.ref_z, z);
                c4 = pid(2, s.ref_yaw, s.yaw_sum);
                c2 = C.sway_slow;
            } else if (range < C.lost && !s.turn) {                    // past the edge: a quarter turn begins
                s.completed_turn = 0;
                s.status = 2;
                s.ref_yaw = rn_add(s.ref_yaw, kHalfPi);
                c3 = pid(1, s.ref_z, z);
                c4 = pid(2, s.ref_yaw, s.yaw_sum);
                s.turn = 1;
            } else if (s.turn && !s.completed_turn) {                  // turning
                s.status = 2;
                c3 = pid(1, s.ref_z, z);
                c4 = pid(2, s.ref_yaw, s.yaw_sum);
                if (fabs(rn_add(s.ref_yaw, -s.yaw_sum)) < C.yaw_tol) {
                    s.completed_turn = 1;
                    if (fabs(rn_add(yaw, -C.yaw0)) < C.yaw_home_tol) {
                        s.completed_round = 1;
                        s.cycle_counter++;
                        if (stats) t.rounds++;
                        if (fabs(rn_add(s.ref_z, -F(C.z_goal))) < C.height_tol) s.completed_mission = 1;
                    } else s.completed_round = 0;
                }
            } else if (range < C.lost && s.completed_turn) {           // turned: look for the next face
                s.status = 3;
                c1 = C.surge_search;
                c2 = C.sway;
                c3 = pid(1, s.ref_z, z);
                c4 = pid(2, s.ref_yaw, s.yaw_sum);
            } else if (in_band && s.completed_turn && s.completed_round) {   // a round is complete: climb
                s.status = 4;
                if (s.get_height) {
                    s.ref_z = rn_add(s.ref_z, C.dz_round);
                    s.ref_x = C.safety_dis;
                    c3 = pid(1, s.ref_z, z);
                    c4 = pid(2, s.ref_yaw, s.yaw_sum);
                    s.get_height = 0;
                } else {
                    s.ref_x = C.safety_dis;
                    c3 = pid(1, s.ref_z, z);
                    c4 = pid(2, s.ref_yaw, s.yaw_sum);
                    if (fabs(rn_add(s.ref_z, -z)) < C.z_tol) s.completed_round = 0;
                }
            } else {                                                   // the node's "state machine failed!"
                failed = true;
                s.status = 2;
                c3 = pid(1, s.ref_z, z);
                c4 = pid(2, s.ref_yaw, s.yaw_sum);
                if (fabs(rn_add(s.ref_yaw, -s.yaw_sum)) < C.yaw_tol) s.completed_turn = 1;
            }
        } else {
            s.status = 5;
            c3 = pid(1, s.ref_z, z);
            c4 = pid(2, s.ref_yaw, s.yaw_sum);
        }
        if (stats) {
#pragma unroll
            for (int i = 0; i < 6; i++) t.ticks[i] += s.status == i ? 1 : 0;
            if (failed) t.failed += 1;
            if (s.completed_mission && t.first_done < 0) t.first_done = (int32_t)k;
            if (s.status == 0) { const double e = rn_add(range, -C.safety_dis); t.standoff_sq = rn_add(t.standoff_sq, rn_mul(e, e)); }
        }
    }
    // the record: u0 = (c1, c2, -c3, c4) and the solver's allocation of it (qp/qp_body.hpp: the same operation order as the host helper)
    rec.u0[0] = c1; rec.u0[1] = c2; rec.u0[2] = -c3; rec.u0[3] = c4;
    rec.cost = 0.0; rec.kkt = 0.0; rec.status = BROV_STATUS_SUCCESS; rec.qp_iter = 0;
    rec.thrust[0] = rn_add(rn_add(-c1, c2), c4) / kRotor;
    rec.thrust[1] = rn_add(rn_add(-c1, -c2), -c4) / kRotor;
    rec.thrust[2] = rn_add(rn_add(c1, c2), -c4) / kRotor;
    rec.thrust[3] = rn_add(rn_add(c1, -c2), c4) / kRotor;
    rec.thrust[4] = c3 / kRotor;
    rec.thrust[5] = c3 / kRotor;
}

// lane 0 of a tick's wave: the controller on the range r and on z and psi of what the controller sees, everything it writes
__device__ __forceinline__ void inspect_tick_lane0(const brov_inspect_params& C, const InspectDev& D, int b, double r, const double* __restrict__ y,
                                                   brov_result* __restrict__ res) {
    brov_inspect_state s = D.state[b];
    brov_inspect_stats t = D.stats[b];
    brov_result rec;
    inspect_control(C, s, t, true, r, y[(size_t)b * 12 + 2], y[(size_t)b * 12 + 5], rec);
    D.state[b] = s;
    D.stats[b] = t;
    D.range[b] = r;
    D.status[b] = s.status;
    res[b] = rec;
}

}  // namespace brov
