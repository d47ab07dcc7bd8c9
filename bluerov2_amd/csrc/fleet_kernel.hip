// fleet_kernel.hip -- the planning tick of a fleet: V vehicles x C candidates laid over one solver of batch B = V * C, instance
// b = v * C + c = candidate c of vehicle v (include/bluerov2_nmpc.h, brov_fleet_*).  Behind a solve:
//   fleet_select_kernel   per vehicle the cheapest eligible candidate (segmented arg-min over the 104-byte result records)
//   fleet_plant_kernel    the vehicle's plant stepped with the winner's u0 -- or, without a winner, with the input applied last
//   fleet_bcast_kernel    the measured state of every vehicle into x0 of all its candidates
// Under disturbance (brov_vehicle_*):
//   fleet_plant_wrench_kernel    fleet_plant_kernel under a world-frame wrench per vehicle, evaluated for the tick by wrench_eval_kernel
//   fleet_observe_inputs_kernel  what the disturbance observer is fed per vehicle: measured state, thrust allocation of the input given, acceleration
//   fleet_apply_kernel           the observer's estimate of vehicle v into p[0..3] of every stage of all its candidates
//
// fleet_select_kernel: one wavefront per vehicle, four vehicles per block.  Lane l scans candidates l, l + 64, ... in ascending order, the
// wave folds (cost, index) pairs with shuffles.  Who is eligible and who wins is the one rule of select_device.hpp (result_eligible,
// argmin_fold, wave_argmin): no atomics, no LDS, two calls return the same bytes.  Only `cost` and `status` of a record are read (16 of its
// 104 bytes), then the winner's record once.
//
// fleet_plant_kernel / fleet_plant_wrench_kernel: one lane per vehicle; where its input comes from and what it records is its own
// (fleet_plant_vehicle, fleet_plant_device.hpp, shared with the plant in moving water of fleet_water_kernel.hip), the step between is plant_erk4 (bluerov2_model.hpp), the function plant_kernel calls, without / with a WorldWrench.
#include <hip/hip_runtime.h>

#include "fleet_kernel.hpp"
#include "fleet_plant_device.hpp"   // fleet_plant_vehicle: gather, plant_erk4, record
#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"
#include "select_device.hpp"

namespace brov {

constexpr int kFleetSelectBlock = 256;
constexpr int kFleetSelectWaves = kFleetSelectBlock / 64;

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
        if (result_eligible(st, cost)) argmin_fold(best, bi, cost, c);
    }
    wave_argmin(best, bi);
    bi = __shfl(bi, 0, 64);
    if (lane == 0) winner[v] = bi;
    if (winner_rec && lane < kResultWords) {   // the record as 13 words, one per lane; zeros without a winner
        result_word(winner_rec + v, lane) = bi >= 0 ? result_word(g + (bi >= 0 ? bi : 0), lane) : 0ULL;
    }
}

__global__ __launch_bounds__(128) void fleet_plant_kernel(FleetPlantArgs A) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= A.V) return;
    fleet_plant_vehicle(A, v, NoWorldWrench{});
}

// the same step under the world-frame wrench wv[v][0..5] of this tick (wrench_eval_kernel wrote it: a fleet buffer or the tick's row of the
// wrench log), held over the tick and projected into the body frame at every RK stage (model_f<WorldWrench>)
__global__ __launch_bounds__(128) void fleet_plant_wrench_kernel(FleetPlantArgs A, const double* __restrict__ wv) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= A.V) return;
    const double* __restrict__ w6 = wv + (size_t)v * 6;
    const WorldWrench ww = {w6[0], w6[1], w6[2], w6[3], w6[4], w6[5]};
    fleet_plant_vehicle(A, v, ww);
}

// one thread per double of x0: consecutive threads write consecutive doubles, the C * 12 readers of a vehicle share its 96 bytes
__global__ __launch_bounds__(256) void fleet_bcast_kernel(const double* __restrict__ xv, long long total, int C, double* __restrict__ x0) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long b = t / NX;
    const int j = (int)(t - b * NX);
    x0[t] = xv[(b / C) * NX + j];
}

// measurement assembly for the observer, one lane per vehicle: y12 = the measured state, thrust = the reference's allocation of the input the
// vehicle was given (the expressions of ekf_inputs_from_solver_kernel, in its order), acc = (v - v_prev) / dt with v_prev kept here
__global__ __launch_bounds__(128) void fleet_observe_inputs_kernel(int V, double dt, double inv_rc, const double* __restrict__ xv,
                                                                   const double* __restrict__ u_hold, double* __restrict__ vprev,
                                                                   double* __restrict__ thrust, double* __restrict__ y12, double* __restrict__ acc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const double* xs = xv + (size_t)v * NX;
#pragma unroll
    for (int j = 0; j < NX; j++) y12[(size_t)v * NX + j] = xs[j];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const double vel = xs[6 + j];
        acc[(size_t)v * 6 + j] = (vel - vprev[(size_t)v * 6 + j]) / dt;
        vprev[(size_t)v * 6 + j] = vel;
    }
    const double* uh = u_hold + (size_t)v * NU;
    const double u0 = uh[0], u1 = uh[1], u2 = uh[2], u3 = uh[3];
    double* t = thrust + (size_t)v * 6;
    t[0] = (-u0 + u1 + u3) * inv_rc;
    t[1] = (-u0 - u1 - u3) * inv_rc;
    t[2] = (u0 + u1 - u3) * inv_rc;
    t[3] = (u0 - u1 + u3) * inv_rc;
    t[4] = (-u2) * inv_rc;
    t[5] = (-u2) * inv_rc;
}

// one thread per (instance, stage): p[0..3] := the estimate of the instance's vehicle; p[4..15] are left alone
__global__ __launch_bounds__(256) void fleet_apply_kernel(int B, int C, int stages, const double* __restrict__ mp, double* __restrict__ par) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;   // (B * stages fits an int, as in ekf_apply_kernel: par holds 128 bytes per k)
    if (k >= B * stages) return;
    const int v = k / stages / C;
    double* p = par + (size_t)k * NP;
#pragma unroll
    for (int j = 0; j < 4; j++) p[j] = mp[(size_t)v * 4 + j];
}

void launch_fleet_select(const brov_result* rec, int V, int C, int32_t* winner, brov_result* winner_rec, hipStream_t st) {
    hipLaunchKernelGGL(fleet_select_kernel, dim3((unsigned)((V + kFleetSelectWaves - 1) / kFleetSelectWaves)), dim3(kFleetSelectBlock), 0, st, rec, V,
                       C, winner, winner_rec);
}
void launch_fleet_plant(const FleetPlantArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(fleet_plant_kernel, dim3((unsigned)((a.V + 127) / 128)), dim3(128), 0, st, a);
}
void launch_fleet_plant_wrench(const FleetPlantArgs& a, const double* wv, hipStream_t st) {
    hipLaunchKernelGGL(fleet_plant_wrench_kernel, dim3((unsigned)((a.V + 127) / 128)), dim3(128), 0, st, a, wv);
}
void launch_fleet_observe_inputs(int V, double dt, const double* xv, const double* u_hold, double* vprev, double* thrust, double* y12, double* acc,
                                 hipStream_t st) {
    hipLaunchKernelGGL(fleet_observe_inputs_kernel, dim3((unsigned)((V + 127) / 128)), dim3(128), 0, st, V, dt, 1.0 / kRotor, xv, u_hold, vprev,
                       thrust, y12, acc);
}
void launch_fleet_apply(int V, int C, int stages, const double* mp, double* par, hipStream_t st) {
    const int B = V * C;
    hipLaunchKernelGGL(fleet_apply_kernel, dim3((unsigned)((B * stages + 255) / 256)), dim3(256), 0, st, B, C, stages, mp, par);
}
void launch_fleet_bcast(const double* xv, int V, int C, double* x0, hipStream_t st) {
    const long long total = (long long)V * C * NX;
    hipLaunchKernelGGL(fleet_bcast_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, xv, total, C, x0);
}

}  // namespace brov
