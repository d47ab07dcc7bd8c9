// select_device.hpp -- "which successful record has the lowest cost", written once for every kernel that answers it: select_best_kernel
// (nmpc_api.hip), group_select_kernel / group_pack_kernel (group_api.hip) and fleet_select_kernel (fleet_kernel.hip).  The rule is the one
// tests/fleet_restatement.py states (DESIGN.md sections 4.11 and 4.12):
//   eligible   status SUCCESS and a finite cost: NaN, +Inf and -Inf never win
//   winner     the eligible record of the lowest cost, on equal cost (-0.0 == 0.0) the lowest index; index -1 when none is eligible
// The lower cost and, on equal cost, the lower index is a total order on (cost, index) pairs, so the winner is a function of the record set:
// it does not depend on how a reduction is cut into lanes, waves and blocks.  No atomics; two launches return the same bytes.
// Device code only, header only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bluerov2_nmpc.h"

namespace brov {

static_assert(sizeof(brov_result) == 104 && sizeof(brov_result) % 8 == 0, "brov_result is copied as 13 words of 8 bytes");
constexpr int kResultWords = (int)(sizeof(brov_result) / 8);

// word w < kResultWords of a record: a record is copied by kResultWords lanes, one word each
__device__ __forceinline__ const unsigned long long& result_word(const brov_result* r, int w) { return reinterpret_cast<const unsigned long long*>(r)[w]; }
__device__ __forceinline__ unsigned long long& result_word(brov_result* r, int w) { return reinterpret_cast<unsigned long long*>(r)[w]; }

// finite is tested on the exponent bits, as track_accumulate_kernel does (an ordering comparison is false for NaN on either side)
__device__ __forceinline__ bool result_eligible(int status, double cost) {
    return status == BROV_STATUS_SUCCESS && (__double2hiint(cost) & 0x7ff00000) != 0x7ff00000;
}

// (c, i) := the better of (c, i) and (c2, i2); i < 0: no candidate yet.  The lower cost, on equal cost the lower index.
__device__ __forceinline__ void argmin_fold(double& c, int& i, double c2, int i2) {
    if (i2 >= 0 && (i < 0 || c2 < c || (c2 == c && i2 < i))) { c = c2; i = i2; }
}

// argmin_fold for a thread's own scan in ascending index order (i2 is above every index it has folded before): an equal cost never replaces
// the earlier index, so the index compare drops out.  The block kernels' scans are latency bound, one wave per SIMD, and pay for every
// instruction in the loop; fleet_select_kernel's scan uses argmin_fold itself.
__device__ __forceinline__ void argmin_next(double& c, int& i, double c2, int i2) {
    if (i < 0 || c2 < c) { c = c2; i = i2; }
}

// the fold of a whole wavefront's pairs, left in lane 0: after the step with offset `off` the lanes below `off` hold the fold of their residue
// class.  Shuffles only; the wavefront calls it as a whole.
__device__ __forceinline__ void wave_argmin(double& c, int& i) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double c2 = __shfl_down(c, off, 64);
        const int i2 = __shfl_down(i, off, 64);
        if (lane + off < 64) argmin_fold(c, i, c2, i2);
    }
}

// the fold of a whole block of kBlock threads, handed to every thread: wave_argmin, then the waves' results meet in LDS.  The block is launched
// with exactly kBlock threads, calls it as a whole and may call it again (the barrier ahead of the stores waits for the readers of the call before).
template <int kBlock>
__device__ __forceinline__ void block_argmin(double& c, int& i) {
    static_assert(kBlock % 64 == 0 && kBlock <= 1024, "whole wavefronts");
    constexpr int kWaves = kBlock / 64;
    __shared__ double sc[kWaves];
    __shared__ int si[kWaves];
    wave_argmin(c, i);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sc[threadIdx.x >> 6] = c; si[threadIdx.x >> 6] = i; }
    __syncthreads();
    c = sc[0]; i = si[0];
#pragma unroll
    for (int w = 1; w < kWaves; w++) argmin_fold(c, i, sc[w], si[w]);
}

}  // namespace brov
