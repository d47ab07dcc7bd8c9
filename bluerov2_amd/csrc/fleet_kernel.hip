// fleet_kernel.hip -- the planning tick of a fleet: V vehicles x C candidates laid over one solver of batch B = V * C, instance
// b = v * C + c = candidate c of vehicle v (include/bluerov2_nmpc.h, brov_fleet_*).  Behind a solve:
//   fleet_select_kernel   per vehicle the cheapest eligible candidate (segmented arg-min over the 104-byte result records)
//   fleet_plant_kernel    the vehicle's plant stepped with the winner's u0 -- or, without a winner, with the input applied last
//   fleet_bcast_kernel    the measured state of every vehicle into x0 of all its candidates
//
// fleet_select_kernel: one wavefront per vehicle, four vehicles per block.  Lane l scans candidates l, l + 64, ... in ascending order, the
// wave folds (cost, index) pairs with shuffles; at every level the lower cost wins and on equal cost the lower index.  That is a total
// order on the pairs, so the result does not depend on how the fold is cut: no atomics, no LDS, two calls return the same bytes.  Only
// `cost` and `status` of a record are read (16 of its 104 bytes), then the winner's record once.  Eligible: status SUCCESS and a finite cost,
// tested on the exponent bits as track_accumulate_kernel does (an ordering comparison is false for NaN on either side).
//
// fleet_plant_kernel: one lane per vehicle; where its input comes from and what it records is its own, the step between is plant_erk4
// (bluerov2_model.hpp), the function plant_kernel calls.
#include <hip/hip_runtime.h>

#include "fleet_kernel.hpp"
#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"

static_assert(sizeof(brov_result) == 104 && sizeof(brov_result) % 8 == 0, "brov_result is copied as 13 words of 8 bytes");

namespace brov {

constexpr int kFleetSelectBlock = 256;
constexpr int kFleetSelectWaves = kFleetSelectBlock / 64;
constexpr int kResultWords = (int)(sizeof(brov_result) / 8);

__device__ __forceinline__ bool fleet_finite(double v) { return (__double2hiint(v) & 0x7ff00000) != 0x7ff00000; }

// (c, i) := the better of (c, i) and (c2, i2); i < 0: no candidate yet.  The lower cost, on equal cost the lower index.
__device__ __forceinline__ void fleet_fold(double& c, int& i, double c2, int i2) {
    if (i2 >= 0 && (i < 0 || c2 < c || (c2 == c && i2 < i))) { c = c2; i = i2; }
}

__global__ __launch_bounds__(kFleetSelectBlock) void fleet_select_kernel(const brov_result* __restrict__ rec, int V, int C,
                                                                         int32_t* __restrict__ winner, brov_result* __restrict__ winner_rec) {
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * kFleetSelectWaves + (threadIdx.x >> 6);
    if (v >= V) return;   // whole wavefronts leave: the shuffles below stay inside one
    const brov_result* __restrict__ g = rec + (size_t)v * C;
    double best = 0.0;
    int bi = -1;
    for (int c = lane; c < C; c += 64) {   // ascending: within a lane an equal cost never replaces an earlier index
        const double cost = g[c].cost;
        const int st = g[c].status;
        if (st == BROV_STATUS_SUCCESS && fleet_finite(cost)) fleet_fold(best, bi, cost, c);
    }
    // after the step with offset `off` the lanes below `off` hold the fold of their residue class
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double c2 = __shfl_down(best, off, 64);
        const int i2 = __shfl_down(bi, off, 64);
        if (lane + off < 64) fleet_fold(best, bi, c2, i2);
    }
    bi = __shfl(bi, 0, 64);
    if (lane == 0) winner[v] = bi;
    if (winner_rec && lane < kResultWords) {   // the record as 13 words, one per lane; zeros without a winner
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(g + (bi >= 0 ? bi : 0));
        reinterpret_cast<unsigned long long*>(winner_rec + v)[lane] = bi >= 0 ? src[lane] : 0ULL;
    }
}

__global__ __launch_bounds__(128) void fleet_plant_kernel(FleetPlantArgs A) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= A.V) return;
    const int win = A.winner[v];
    const brov_result* __restrict__ g = A.res + (size_t)v * A.C;
    const double* usrc;
    int status = BROV_STATUS_SUCCESS;
    if (win >= 0) {
        usrc = g[win].u0;
    } else {
        // zero-order hold: the input applied last (zeros after a reset); the status is candidate 0's, or NAN where candidate 0 reported
        // success with a cost that is not finite
        usrc = A.u_hold + (size_t)v * NU;
        const int s0 = g[0].status;
        status = s0 != BROV_STATUS_SUCCESS ? s0 : BROV_STATUS_NAN;
    }
    double x[NX], u[NU];
    ModelPar m;
    Wrench w;
    plant_inputs(A.xv + (size_t)v * NX, usrc, A.pp + (size_t)v * A.pp_stride, nullptr, 0, x, u, m, w);
    plant_erk4(x, w, m, NoWorldWrench{}, A.dt, A.substeps);
    store_row(A.xv + (size_t)v * NX, x);
    store_row(A.u_hold + (size_t)v * NU, u);
    A.status[v] = status;
    log_row(A.xlog, v, x);
    log_row(A.ulog, v, u);
    if (A.stlog) A.stlog[v] = status;
    if (A.winlog) A.winlog[v] = win;
}

// one thread per double of x0: consecutive threads write consecutive doubles, the C * 12 readers of a vehicle share its 96 bytes
__global__ __launch_bounds__(256) void fleet_bcast_kernel(const double* __restrict__ xv, long long total, int C, double* __restrict__ x0) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long b = t / NX;
    const int j = (int)(t - b * NX);
    x0[t] = xv[(b / C) * NX + j];
}

void launch_fleet_select(const brov_result* rec, int V, int C, int32_t* winner, brov_result* winner_rec, hipStream_t st) {
    hipLaunchKernelGGL(fleet_select_kernel, dim3((unsigned)((V + kFleetSelectWaves - 1) / kFleetSelectWaves)), dim3(kFleetSelectBlock), 0, st, rec, V,
                       C, winner, winner_rec);
}
void launch_fleet_plant(const FleetPlantArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(fleet_plant_kernel, dim3((unsigned)((a.V + 127) / 128)), dim3(128), 0, st, a);
}
void launch_fleet_bcast(const double* xv, int V, int C, double* x0, hipStream_t st) {
    const long long total = (long long)V * C * NX;
    hipLaunchKernelGGL(fleet_bcast_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, xv, total, C, x0);
}

}  // namespace brov
