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
