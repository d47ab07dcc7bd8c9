// rotor_kernel.hip -- the rotor stage of the solver's plant (include/bluerov2_nmpc.h, brov_rotor_*): every thruster answers its command with
// first-order dynamics r' = (c - r) / tau (the reference's vehicle: FirstOrder, timeConstant 0.2 s, a command clamp ahead of the dynamics).
// Its place in the chain is delay -> rotor -> thruster stage (clip / fault / K) -> model: the kernel runs ahead of the plant kernel in force
// and rewrites the record that kernel reads; no plant kernel knows of it.
// Per instance b and thruster i, with the state r = r[b][i] (zero when the stage is set or reset), the command t = rec[b].thrust[i] and the
// coefficients alpha = alpha[b][i], beta = beta[b][i] the HOST computed (brov_rotor_coeffs: alpha = exp(-h / tau), beta = (1 - alpha) / (h / tau);
// tau = 0 gives the pair (0, 0)) -- no device exp stands between this kernel and tests/rotor_restatement.py:
//     c  = t < lo[i] ? lo[i] : (t > hi[i] ? hi[i] : t)          the thruster stage's clip expression
//     if !isfinite(c): c = r                                    a non-finite command moves nothing and is never stored
//     d  = r + (-c)
//     m  = c + beta  * d                                        mean thrust over the step: what the plant is given (zero-order hold)
//     r' = c + alpha * d                                        the state at the end of the step
// every operation rounded on its own (rn_mul / rn_add of rounded_ops.hpp under `fp contract(off)`): four roundings for m and r' together
// besides the sign flip.  A pair (alpha, beta) == (0, 0) COPIES m = r' = c (c + 0 * d would turn -0 into +0).
// The applied record is the record received with thrust[i] = m[i] and u0 = the allocation's left inverse of m, rc = kRotor, in this order:
//     u0[0] = (rc * (((-m0 + -m1) +  m2) +  m3)) * 0.25
//     u0[1] = (rc * ((( m0 + -m1) +  m2) + -m3)) * 0.25
//     u0[3] = (rc * ((( m0 + -m1) + -m2) +  m3)) * 0.25
//     u0[2] = -((rc * (m4 + m5)) * 0.5)
// so that the plant without the thruster stage and the observer (ekf_inputs_from_solver_kernel), which both read u0, see the lagged forces.
// An instance whose six pairs are all (0, 0) and whose six c have the bits of their t (no limit acted, no command was non-finite) keeps
// its u0: the whole record is copied bit for bit.
// Bookkeeping per step: last[b][i] = m[i]; lag_sq[b] += sum_i (c[i] - m[i])^2, six squares summed in index order, then ONE add into the sum,
// as thruster_account does it.  A `u` log row gets the COMMANDED u0 of the record received (under the delay stage that stage has written it
// and none is passed).  The thruster stage behind this one counts the lagged thrusts m as its "commanded" in clip_ticks and lost_sq.
// rotor_shift_kernel advances the state and keeps the books; rotor_eval_kernel takes commands and a state, returns the applied thrusts and
// the new state and moves nothing.  Both: one lane per instance, 128-thread blocks, FP64, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"   // kRotor
#include "rounded_ops.hpp"      // rn_mul, rn_add

namespace brov {

// one step of the six rotors of instance b: c (the commands that count), m (applied), rn (new state) from t (commands) and r (state)
__device__ __forceinline__ void rotor_stage(const RotorPar& P, const double* __restrict__ alpha, const double* __restrict__ beta, int b,
                                            const double (&t)[6], const double (&r)[6], double (&c)[6], double (&m)[6], double (&rn)[6],
                                            bool* untouched) {
#pragma clang fp contract(off)
    bool same = true;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double al = alpha[(size_t)b * 6 + i], be = beta[(size_t)b * 6 + i];
        double ci = t[i] < P.lo[i] ? P.lo[i] : (t[i] > P.hi[i] ? P.hi[i] : t[i]);
        if (!isfinite(ci)) ci = r[i];
        const bool copy = al == 0.0 && be == 0.0;
        const double d = rn_add(r[i], -ci);
        c[i] = ci;
        m[i] = copy ? ci : rn_add(ci, rn_mul(be, d));
        rn[i] = copy ? ci : rn_add(ci, rn_mul(al, d));
        same = same && copy && __double_as_longlong(ci) == __double_as_longlong(t[i]);
    }
    *untouched = same;
}

__global__ __launch_bounds__(128) void rotor_shift_kernel(const brov_result* __restrict__ rec, brov_result* __restrict__ applied, RotorPar P,
                                                          const double* __restrict__ alpha, const double* __restrict__ beta,
                                                          double* __restrict__ state, double* __restrict__ last, double* __restrict__ lag_sq,
                                                          int B, double* __restrict__ ulog) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    brov_result q = rec[b];
    double t[6], r[6], c[6], m[6], rn[6];
#pragma unroll
    for (int i = 0; i < 6; i++) { t[i] = q.thrust[i]; r[i] = state[(size_t)b * 6 + i]; }
    if (ulog) {
#pragma unroll
        for (int j = 0; j < 4; j++) ulog[(size_t)b * 4 + j] = q.u0[j];
    }
    bool untouched;
    rotor_stage(P, alpha, beta, b, t, r, c, m, rn, &untouched);
    double sq = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double d = rn_add(c[i], -m[i]);
        sq = i == 0 ? rn_mul(d, d) : rn_add(sq, rn_mul(d, d));
        state[(size_t)b * 6 + i] = rn[i];
        last[(size_t)b * 6 + i] = m[i];
        q.thrust[i] = m[i];
    }
    lag_sq[b] = rn_add(lag_sq[b], sq);
    if (!untouched) {
        q.u0[0] = rn_mul(rn_mul(kRotor, rn_add(rn_add(rn_add(-m[0], -m[1]), m[2]), m[3])), 0.25);
        q.u0[1] = rn_mul(rn_mul(kRotor, rn_add(rn_add(rn_add(m[0], -m[1]), m[2]), -m[3])), 0.25);
        q.u0[3] = rn_mul(rn_mul(kRotor, rn_add(rn_add(rn_add(m[0], -m[1]), -m[2]), m[3])), 0.25);
        q.u0[2] = -rn_mul(rn_mul(kRotor, rn_add(m[4], m[5])), 0.5);
    }
    applied[b] = q;
}

__global__ __launch_bounds__(128) void rotor_eval_kernel(RotorPar P, const double* __restrict__ alpha, const double* __restrict__ beta,
                                                         const double* __restrict__ commanded, const double* __restrict__ state,
                                                         double* __restrict__ applied, double* __restrict__ state_out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double t[6], r[6], c[6], m[6], rn[6];
#pragma unroll
    for (int i = 0; i < 6; i++) { t[i] = commanded[(size_t)b * 6 + i]; r[i] = state[(size_t)b * 6 + i]; }
    bool untouched;
    rotor_stage(P, alpha, beta, b, t, r, c, m, rn, &untouched);
#pragma unroll
    for (int i = 0; i < 6; i++) { applied[(size_t)b * 6 + i] = m[i]; state_out[(size_t)b * 6 + i] = rn[i]; }
}

void launch_rotor_shift(const brov_result* rec, brov_result* applied, const RotorPar& P, const double* alpha, const double* beta, double* state,
                        double* last, double* lag_sq, int B, double* ulog, hipStream_t st) {
    hipLaunchKernelGGL(rotor_shift_kernel, dim3((B + 127) / 128), dim3(128), 0, st, rec, applied, P, alpha, beta, state, last, lag_sq, B, ulog);
}
void launch_rotor_eval(const RotorPar& P, const double* alpha, const double* beta, const double* commanded, const double* state, double* applied,
                       double* state_out, int B, hipStream_t st) {
    hipLaunchKernelGGL(rotor_eval_kernel, dim3((B + 127) / 128), dim3(128), 0, st, P, alpha, beta, commanded, state, applied, state_out, B);
}

}  // namespace brov
