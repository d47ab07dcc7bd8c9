// inspect_kernel.hip -- the bridge-pier inspection loop (brov_range_*, brov_inspect_*; include/bluerov2_nmpc_inspect.h has the formulas): the
// depth camera's mean range against axis-aligned boxes, and the reference's VisualController -- a six-state mission machine with three PID
// loops (bluerov2_dobmpc/src/bluerov2_inspection_node.cpp:289-532, restated from reading it) -- which writes the solver's own result records.
//   range_eval_kernel    the range stage alone: one wavefront per instance, roi * roi rays against K boxes, no atomics
//   inspect_eval_kernel  the controller alone: one lane per instance
//   inspect_tick_kernel  one tick of the loop: the wave casts the rays from the true state, lane 0 runs the controller on what the controller
//                        sees of z and psi and writes record, state, statistics, last range and status
// The bodies -- rotation, rays, box loop, tree sum, controller -- live in range_device.hpp, which mesh_kernel.hip shares: with a triangle mesh
// in the scene (brov_mesh_*) its kernels run in place of range_eval_kernel and inspect_tick_kernel.
// The scene and the camera are kernel arguments: wave-uniform, read with scalar loads.  The instance of a wave is made uniform with
// readfirstlane, so its state is read with scalar loads as well.  Per ray: the direction, its three reciprocals (once, not per box) and the
// range factor sqrt(1 + a^2 + b^2); per ray-box pair 6 products, 6 min / max and 3 compares on wave-uniform differences lo - o, hi - o.
// Every operation is rounded on its own (fp contract off for the whole file; the sums and products tests/inspect_restatement.py restates
// bit for bit are written with rn_add / rn_mul), the quotients are IEEE divisions, the square root is __dsqrt_rn.  FP64, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "range_device.hpp"

#pragma clang fp contract(off)

namespace brov {

// ---- kernels: 256 threads = 4 wavefronts = 4 instances per block -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void range_eval_kernel(brov_range_params P, RangeScene S, const double* __restrict__ sigma, int B, int m,
                                                         const double* __restrict__ x, double* __restrict__ range, int32_t* __restrict__ hits,
                                                         double* __restrict__ rot, double* __restrict__ depth) {
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
    if (b >= B) return;
    double r;
    int n;
    range_wave_on<false>(P, S, MeshDev{}, sigma, b, m, lane, x + (size_t)b * 12, rot, depth, r, n, nullptr);
    if (lane == 0) { range[b] = r; hits[b] = n; }
}

__global__ __launch_bounds__(128) void inspect_eval_kernel(brov_inspect_params C, int B, const brov_inspect_state* __restrict__ state_in,
                                                           const double* __restrict__ range, const double* __restrict__ z,
                                                           const double* __restrict__ psi, brov_inspect_state* __restrict__ state_out,
                                                           brov_result* __restrict__ rec, brov_inspect_stats* stats) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    brov_inspect_state s = state_in[b];
    brov_inspect_stats t = {};
    if (stats) t = stats[b];
    brov_result r;
    inspect_control(C, s, t, stats != nullptr, range[b], z[b], psi[b], r);
    state_out[b] = s;
    rec[b] = r;
    if (stats) stats[b] = t;
}

__global__ __launch_bounds__(256) void inspect_tick_kernel(brov_range_params P, RangeScene S, const double* __restrict__ sigma, brov_inspect_params C,
                                                           InspectDev D, int B, int m, const double* __restrict__ x, const double* __restrict__ y,
                                                           brov_result* __restrict__ res) {
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
    if (b >= B) return;
    double r;
    int n;
    range_wave_on<false>(P, S, MeshDev{}, sigma, b, m, lane, x + (size_t)b * 12, nullptr, nullptr, r, n, nullptr);
    if (lane != 0) return;
    inspect_tick_lane0(C, D, b, r, y, res);
}

void launch_range_eval(const brov_range_params& P, const RangeScene& S, const double* sigma, int B, long long m, const double* x, double* range,
                       int32_t* hits, double* rot, double* depth, hipStream_t st) {
    hipLaunchKernelGGL(range_eval_kernel, dim3((B + 3) / 4), dim3(256), 0, st, P, S, sigma, B, (int)m, x, range, hits, rot, depth);
}
void launch_inspect_eval(const brov_inspect_params& C, int B, const brov_inspect_state* state_in, const double* range, const double* z,
                         const double* psi, brov_inspect_state* state_out, brov_result* rec, brov_inspect_stats* stats, hipStream_t st) {
    hipLaunchKernelGGL(inspect_eval_kernel, dim3((B + 127) / 128), dim3(128), 0, st, C, B, state_in, range, z, psi, state_out, rec, stats);
}
void launch_inspect_tick(const brov_range_params& P, const RangeScene& S, const double* sigma, const brov_inspect_params& C, const InspectDev& D,
                         int B, long long m, const double* x, const double* y, brov_result* res, hipStream_t st) {
    hipLaunchKernelGGL(inspect_tick_kernel, dim3((B + 3) / 4), dim3(256), 0, st, P, S, sigma, C, D, B, (int)m, x, y, res);
}

}  // namespace brov
