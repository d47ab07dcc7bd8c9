// current_gen.hpp -- the device side of the ocean current's generator (brov_current_* of include/bluerov2_nmpc.h), shared by the plant kernels
// that integrate in moving water: plant_current.hip and plant_coriolis.hip.  Written with the singly rounded operations of rounded_ops.hpp:
// the kernels and the numpy restatement of tests/current_restatement.py agree bit for bit.  Device code.
#pragma once
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "plant_stages.hpp"   // counter_uniform

namespace brov {

// the current of instance b at tick k: Gauss-Markov mode: the state as it stands
__device__ __forceinline__ void current_at(const CurrentGen& g, int b, long long k, double (&v)[3]) {
    if (g.mode == BROV_CURRENT_CONSTANT) {
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = g.v[(size_t)b * 3 + i];
    } else if (g.mode == BROV_CURRENT_TABLE) {
        long long r = k < 0 ? 0 : k;
        if (r > g.rows - 1) r = g.rows - 1;   // past the end: the last row, repeated, as the wrench table does
        const double gn = g.gain ? g.gain[b] : 1.0;
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = rn_mul(g.tab[(size_t)r * 3 + i], gn);
    } else if (g.mode == BROV_CURRENT_GAUSS_MARKOV) {
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = g.c[(size_t)b * 3 + i];
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = 0.0;
    }
}

// c <- the Gauss-Markov state one tick later, drawn at counter tick k (0 <= k < 2^22, the host has checked): per axis
//   v = (c - step * (mu * (c - mean))) + amp * (2 U - 1), clamped to [lo, hi]; every operation rounded on its own
__device__ __forceinline__ void current_advance(const CurrentGen& g, int b, long long k, const double (&c)[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double U = counter_uniform(g.seed, b, k, i);   // (channel 3 stays reserved, as in the wrench's draw)
        const double xi = rn_add(rn_mul(2.0, U), -1.0);
        const double pull = rn_mul(g.step, rn_mul(g.mu[i], rn_add(c[i], -g.mean[(size_t)b * 3 + i])));
        const double v = rn_add(rn_add(c[i], -pull), rn_mul(g.amp[i], xi));
        g.c[(size_t)b * 3 + i] = v < g.lo[i] ? g.lo[i] : (v > g.hi[i] ? g.hi[i] : v);
    }
}

}  // namespace brov
