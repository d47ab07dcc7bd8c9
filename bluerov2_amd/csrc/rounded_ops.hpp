// rounded_ops.hpp -- what the stateless stages of the plant (plant_wrench.hip: wrench generator, thruster stage; sensor_kernel.hip: sensor
// stage) share so that a numpy restatement agrees with them bit for bit: the counter hash and the two singly rounded operations.  Device code.
#pragma once
#include <hip/hip_runtime.h>

namespace brov {

// the output function of SplitMix64 (Steele, Lea, Flood 2014; public domain reference implementation by S. Vigna)
__device__ __forceinline__ unsigned long long splitmix64_finalise(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// the counter hash and the Irwin-Hall(12) variate of the sensor stages (sensor_kernel.hip states the construction): instance b, measurement
// index m (24 bits), channel slot c (6 bits: 0..12 the sensor stage, 16..28 the IMU/GPS stage), j = 0, 1, 2
__device__ __forceinline__ unsigned long long sensor_hash(unsigned long long seed, int b, int m, int c, int j) {
    const unsigned long long k = ((unsigned long long)b << 32) | ((unsigned long long)m << 8) | ((unsigned long long)c << 2) | (unsigned long long)j;
    return splitmix64_finalise((seed ^ 0x53454E534F52ULL) + (k + 1ULL) * 0x9E3779B97F4A7C15ULL);
}
__device__ __forceinline__ double sensor_noise(unsigned long long seed, int b, int m, int c) {
    int S = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const unsigned long long h = sensor_hash(seed, b, m, c, j);
        S += (int)(h & 0xFFFF) + (int)((h >> 16) & 0xFFFF) + (int)((h >> 32) & 0xFFFF) + (int)(h >> 48);
    }
    return (double)(S - 393210) * 0x1.0p-16;   // exact: |S - 393210| < 2^19
}

// rn_mul / rn_add: one product / one sum, rounded to nearest, that no caller's context fuses.  __dmul_rn / __dadd_rn do not give that here: the header defines
// them as inline functions `x * y` / `x + y` compiled OUTSIDE a caller's `fp contract(off)`, so their instructions carry the contract flag
// into the caller, and a stage written with them compiled to 36 v_fmac_f64 (wrench_at's two products happen to be exact or added to zero
// in every test).  Written here under the pragma, the instructions carry no such flag wherever they are inlined.
__device__ __forceinline__ double rn_mul(double p, double q) {
#pragma clang fp contract(off)
    return p * q;
}
__device__ __forceinline__ double rn_add(double p, double q) {
#pragma clang fp contract(off)
    return p + q;
}

}  // namespace brov
