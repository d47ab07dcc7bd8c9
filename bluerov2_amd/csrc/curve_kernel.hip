// curve_kernel.hip -- the thrust-curve stage of the solver's plant (include/bluerov2_nmpc_curve.h, brov_curve_*): what stands between a wanted
// thrust and the force a thruster gives besides its lag.  Its place in the chain is
//     delay -> [COMMAND part] -> rotor -> [THRUST part] -> thruster stage (clip / fault / K) -> model
// The COMMAND part is the controller's side (pre-map, quantisation to the ESC's steps), the THRUST part the thruster's (conversion curve,
// efficiency): dynamics on the command, then conversion, the order of the reference's vehicle.  With the rotor stage off the two are adjacent
// and run as ONE launch (BOTH), which is DEFINED as COMMAND followed by THRUST, bit for bit, the rewritten u0 included.
// Per instance b and thruster i, t = rec[b].thrust[i], every operation rounded on its own (rn_mul / rn_add of rounded_ops.hpp under
// `fp contract(off)`), no transcendental, no division, no reciprocal on the device:
//   COMMAND   w = t                                              PRE_NONE
//             w = (((p0 t + p1) t + p2) t + p3) t + p4           PRE_POLY, Horner, highest degree first
//             w = lookup(pre table, t)                           PRE_TABLE
//             quantum > 0:  w = quantum * rint(w * inv_quantum)  rint: ties to even; inv_quantum from the host
//   THRUST    f = w                                              LINEAR (a copy: -0 stays -0)
//             f = k * (w * |w|)                                  BASIC
//             v = w * |w|;  f = v <= dl ? kl * (v + (-dl)) : (v >= dr ? kr * (v + (-dr)) : +0.0)      DEADZONE
//             f = lookup(curve table, w)                         TABLE
//             f = eff[b][i] * f  unless eff[b][i] == 1.0, which copies
//   lookup    knots x[0..K) strictly increasing, (y, slope) pairs with the slopes from the HOST: w <= x[0] or w >= x[K-1] gives y[0] / y[K-1];
//             else j = the largest index with x[j] <= w and the value is y[j] + slope[j] * (w + (-x[j])).  The amps column is interpolated
//             with the same j and the same expression.
//   NaN       a NaN input of a part is its output, bit for bit; a NaN that a part makes of another input (0 * inf, inf - inf) is the one
//             quiet NaN 0x7FF8000000000000, so that the result does not depend on whose hardware made it.
// The applied record of a part is the record received with thrust = its output; where a bit of the six changed, u0 = the allocation's left
// inverse of the output, in the operation order rotor_kernel.hip writes down (restated here: that file is left as it is); else the record is
// copied whole.  BOTH rewrites u0 where either part changed a bit.
// Books per plant step: wanted = t ahead of COMMAND, last_command = w, last_thrust = f, err_sq[b] += sum_i (wanted_i - f_i)^2 (six squares
// summed in index order, then ONE add, as thruster_account does it), dead_ticks[b][i] += (f_i == 0 && wanted_i != 0), and with an amps column
// charge[b] += dt * sum_i amps_i.
// One lane per instance, 128-thread blocks, FP64, no scratch.  The tables are the batch's: a block stages the images it needs once in LDS
// (dynamic: a launch whose modes use no table asks for none) and every lane searches there, eight fixed halving steps over x with 8-byte reads
// (lanes stand on different knots: a b64 read's conflicts stay within a 32-lane half, and equal knots broadcast), then the (y, slope) pair,
// which lies together on 16 bytes (the compiler reads it as two b64 today; the layout leaves a b128 open).
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"   // kRotor
#include "rounded_ops.hpp"      // rn_mul, rn_add
#include "../../include/bluerov2_nmpc.h"

namespace brov {

struct CurveTable {   // a staged image (nmpc_device.hpp, curve_image_doubles)
    const double* x;
    const double2* ys;
    const double2* as;
    int K;
};
__device__ __forceinline__ CurveTable curve_table_at(const double* base, int K, bool amps) {
    const int Ke = (K + 1) & ~1;
    CurveTable T;
    T.x = base; T.ys = (const double2*)(base + Ke); T.as = amps ? (const double2*)(base + Ke + 2 * K) : nullptr; T.K = K;
    return T;
}

// a NaN input is the output; a NaN made of another input is the one quiet NaN
__device__ __forceinline__ double nan_rule(double out, double in) {
    return in != in ? in : (out != out ? __longlong_as_double(0x7FF8000000000000LL) : out);
}

template <bool AMPS>
__device__ __forceinline__ double curve_lookup(const CurveTable& T, double w, double* amps) {
#pragma clang fp contract(off)
    int j = 0;
#pragma unroll
    for (int s = 128; s; s >>= 1) {
        const int c = j + s;
        if (c < T.K && T.x[c] <= w) j = c;
    }
    const bool end = w <= T.x[0] || w >= T.x[T.K - 1];   // the same address in every lane: a broadcast
    const double d = rn_add(w, -T.x[j]);
    const double2 r = T.ys[j];
    if (AMPS) {
        const double2 a = T.as[j];
        *amps = end ? a.x : rn_add(a.x, rn_mul(a.y, d));
    }
    return end ? r.x : rn_add(r.x, rn_mul(r.y, d));
}

__device__ __forceinline__ double curve_command(const CurvePar& P, const CurveTable& pre, double t) {
#pragma clang fp contract(off)
    double w = t;
    if (P.pre == BROV_CURVE_PRE_POLY) {
        w = P.pre_poly[0];
#pragma unroll
        for (int i = 1; i < 5; i++) w = rn_add(rn_mul(w, t), P.pre_poly[i]);
    } else if (P.pre == BROV_CURVE_PRE_TABLE) {
        w = curve_lookup<false>(pre, t, nullptr);
    }
    if (P.quantum > 0.0) w = rn_mul(P.quantum, rint(rn_mul(w, P.inv_quantum)));
    return nan_rule(w, t);
}

__device__ __forceinline__ double curve_thrust(const CurvePar& P, const CurveTable& cur, double e, double w, double* amps) {
#pragma clang fp contract(off)
    double f = w;
    *amps = 0.0;
    if (P.kind == BROV_CURVE_BASIC) {
        f = rn_mul(P.k, rn_mul(w, fabs(w)));
    } else if (P.kind == BROV_CURVE_DEADZONE) {
        const double v = rn_mul(w, fabs(w));
        f = v <= P.dl ? rn_mul(P.kl, rn_add(v, -P.dl)) : (v >= P.dr ? rn_mul(P.kr, rn_add(v, -P.dr)) : 0.0);
    } else if (P.kind == BROV_CURVE_TABLE) {
        if (P.amps) { f = curve_lookup<true>(cur, w, amps); *amps = nan_rule(*amps, w); }
        else f = curve_lookup<false>(cur, w, nullptr);
    }
    if (e != 1.0) f = rn_mul(e, f);
    return nan_rule(f, w);
}

// the images the parts PART need, staged by the whole block; every thread of the block calls it, the tail lanes too
template <int PART>
__device__ __forceinline__ void curve_stage_tables(const CurvePar& P, const double* __restrict__ img_curve, const double* __restrict__ img_pre,
                                                   double* lds, CurveTable* cur, CurveTable* pre) {
    const bool use_cur = (PART & CURVE_THRUST) && P.kind == BROV_CURVE_TABLE;
    const bool use_pre = (PART & CURVE_COMMAND) && P.pre == BROV_CURVE_PRE_TABLE;
    const int nc = use_cur ? curve_image_doubles(P.Kc, P.amps != 0) : 0;
    const int np = use_pre ? curve_image_doubles(P.Kp, false) : 0;
    for (int i = threadIdx.x; i < nc; i += blockDim.x) lds[i] = img_curve[i];
    for (int i = threadIdx.x; i < np; i += blockDim.x) lds[nc + i] = img_pre[i];
    if (nc + np) __syncthreads();   // wave-uniform, block-uniform
    *cur = curve_table_at(lds, P.Kc, P.amps != 0);
    *pre = curve_table_at(lds + nc, P.Kp, false);
}

template <int PART>
__global__ __launch_bounds__(128) void curve_shift_kernel(const brov_result* __restrict__ rec, brov_result* __restrict__ applied, CurvePar P,
                                                          const double* __restrict__ eff, const double* __restrict__ img_curve,
                                                          const double* __restrict__ img_pre, CurveBooks bk, double dt, int B,
                                                          double* __restrict__ ulog) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double curve_lds[];
    CurveTable cur, pre;
    curve_stage_tables<PART>(P, img_curve, img_pre, curve_lds, &cur, &pre);
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    brov_result q = rec[b];
    if (ulog) {
#pragma unroll
        for (int j = 0; j < 4; j++) ulog[(size_t)b * 4 + j] = q.u0[j];
    }
    double o[6], want[6];   // the output of the last part run; what entered the COMMAND part
    bool changed = false;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        o[i] = q.thrust[i];
        want[i] = (PART & CURVE_COMMAND) ? o[i] : bk.wanted[(size_t)b * 6 + i];
    }
    if (PART & CURVE_COMMAND) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double t = o[i];
            o[i] = curve_command(P, pre, t);
            bk.wanted[(size_t)b * 6 + i] = t;
            bk.last_command[(size_t)b * 6 + i] = o[i];
            changed = changed || __double_as_longlong(o[i]) != __double_as_longlong(t);
        }
    }
    if (PART & CURVE_THRUST) {
        double sq = 0.0, amp = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double w = o[i];
            double a;
            o[i] = curve_thrust(P, cur, eff[(size_t)b * 6 + i], w, &a);
            bk.last_thrust[(size_t)b * 6 + i] = o[i];
            changed = changed || __double_as_longlong(o[i]) != __double_as_longlong(w);
            const double d = rn_add(want[i], -o[i]);
            sq = i == 0 ? rn_mul(d, d) : rn_add(sq, rn_mul(d, d));
            amp = i == 0 ? a : rn_add(amp, a);
            if (o[i] == 0.0 && want[i] != 0.0) bk.dead_ticks[(size_t)b * 6 + i] += 1;
        }
        bk.err_sq[b] = rn_add(bk.err_sq[b], sq);
        if (P.kind == BROV_CURVE_TABLE && P.amps) bk.charge[b] = rn_add(bk.charge[b], rn_mul(dt, amp));
    }
    if (changed) {
#pragma unroll
        for (int i = 0; i < 6; i++) q.thrust[i] = o[i];
        // the allocation's left inverse, the operation order of rotor_kernel.hip
        q.u0[0] = rn_mul(rn_mul(kRotor, rn_add(rn_add(rn_add(-o[0], -o[1]), o[2]), o[3])), 0.25);
        q.u0[1] = rn_mul(rn_mul(kRotor, rn_add(rn_add(rn_add(o[0], -o[1]), o[2]), -o[3])), 0.25);
        q.u0[3] = rn_mul(rn_mul(kRotor, rn_add(rn_add(rn_add(o[0], -o[1]), -o[2]), o[3])), 0.25);
        q.u0[2] = -rn_mul(rn_mul(kRotor, rn_add(o[4], o[5])), 0.5);
    }
    applied[b] = q;
}

__global__ __launch_bounds__(128) void curve_eval_kernel(int part, CurvePar P, const double* __restrict__ eff, const double* __restrict__ img_curve,
                                                         const double* __restrict__ img_pre, const double* __restrict__ in,
                                                         double* __restrict__ out, double* __restrict__ amps_out, int B) {
    extern __shared__ __attribute__((aligned(16))) double curve_lds[];
    CurveTable cur, pre;
    if (!(part & CURVE_COMMAND)) P.pre = BROV_CURVE_PRE_NONE;   // a part that does not run stages nothing (wave-uniform)
    if (!(part & CURVE_THRUST)) P.kind = BROV_CURVE_LINEAR;
    curve_stage_tables<CURVE_BOTH>(P, img_curve, img_pre, curve_lds, &cur, &pre);
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double v = in[(size_t)b * 6 + i], a = 0.0;
        if (part & CURVE_COMMAND) v = curve_command(P, pre, v);
        if (part & CURVE_THRUST) v = curve_thrust(P, cur, eff[(size_t)b * 6 + i], v, &a);
        out[(size_t)b * 6 + i] = v;
        amps_out[(size_t)b * 6 + i] = a;
    }
}

// the LDS bytes a launch of `part` asks for: the images its modes use, none else
static size_t curve_lds_bytes(int part, const CurvePar& P) {
    const int nc = (part & CURVE_THRUST) && P.kind == BROV_CURVE_TABLE ? curve_image_doubles(P.Kc, P.amps != 0) : 0;
    const int np = (part & CURVE_COMMAND) && P.pre == BROV_CURVE_PRE_TABLE ? curve_image_doubles(P.Kp, false) : 0;
    return (size_t)(nc + np) * sizeof(double);
}

void launch_curve_shift(int part, const brov_result* rec, brov_result* applied, const CurvePar& P, const double* eff, const double* img_curve,
                        const double* img_pre, const CurveBooks& bk, double dt, int B, double* ulog, hipStream_t st) {
    const dim3 grid((B + 127) / 128), block(128);
    const size_t lds = curve_lds_bytes(part, P);
    if (part == CURVE_COMMAND)
        hipLaunchKernelGGL(curve_shift_kernel<CURVE_COMMAND>, grid, block, lds, st, rec, applied, P, eff, img_curve, img_pre, bk, dt, B, ulog);
    else if (part == CURVE_THRUST)
        hipLaunchKernelGGL(curve_shift_kernel<CURVE_THRUST>, grid, block, lds, st, rec, applied, P, eff, img_curve, img_pre, bk, dt, B, ulog);
    else
        hipLaunchKernelGGL(curve_shift_kernel<CURVE_BOTH>, grid, block, lds, st, rec, applied, P, eff, img_curve, img_pre, bk, dt, B, ulog);
}
void launch_curve_eval(int part, const CurvePar& P, const double* eff, const double* img_curve, const double* img_pre, const double* in, double* out,
                       double* amps_out, int B, hipStream_t st) {
    hipLaunchKernelGGL(curve_eval_kernel, dim3((B + 127) / 128), dim3(128), curve_lds_bytes(part, P), st, part, P, eff, img_curve, img_pre, in, out,
                       amps_out, B);
}

}  // namespace brov
