// clearance_kernel.hpp -- launchers of the inter-vehicle clearance kernels (clearance_kernel.hip) for their host side (fleet_api.hip,
// brov_clearance_*).  The plan is kept STAGE-MAJOR on the device: plan[k][v][0..2], k = 0..N; the host accessors convert.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bluerov2_nmpc.h"

namespace brov {

constexpr int kClearanceMaxSlices = 8;   // grid-level slices of the peer range: part holds [kClearanceMaxSlices][B]

// how many grid-level slices of the peer range a launch at (B, V) takes: enough blocks to give every SIMD of the device two wavefronts where
// the batch alone does not, never more than there are peers to share out.  The result does not depend on it (a minimum has no order).
int clearance_slices(int B, int V);

// part[s][b] = min over the peers w != b / C of slice s and the stages k = 0..N of |x[b][k][0..2] - plan[min(k + shift, N)][w]|^2 (+Inf
// over an empty set); x DEVICE [B][N+1][12], plan DEVICE [N+1][V][3], part DEVICE [slices][B]
void launch_clearance_dist(const double* x, const double* plan, int B, int V, int C, int N, int shift, int slices, double* part, hipStream_t st);

// d2min[b] = min over the slices of part; out (or nullptr) [b] = rec[b] with cost += weight * (r2 - d2min[b]) where d2min[b] < r2
void launch_clearance_rescore(const double* part, int slices, int B, const brov_result* rec, double r2, double weight, double* d2min,
                              brov_result* out, hipStream_t st);

// behind the select: plan[.][v] := the winner's iterate positions, or the old plan advanced by `shift` stages; the statistics of the step
void launch_clearance_publish(const double* x, const int32_t* winner, const double* d2min, int V, int C, int N, int shift, double r2, double* plan,
                              double* last_d2, double* min_d2, int32_t* below, hipStream_t st);

}  // namespace brov
