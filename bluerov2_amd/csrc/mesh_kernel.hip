// mesh_kernel.hip -- the inspection loop against a triangle mesh (brov_mesh_*; include/bluerov2_nmpc_mesh.h has the formulas): the kernels
// InspectSource launches in place of range_eval_kernel and inspect_tick_kernel iff a mesh is set.
//   mesh_eval_kernel          the range stage alone, boxes and mesh, with the per-instance counts of node tests and triangle tests
//   inspect_mesh_tick_kernel  one tick of the loop: the wave casts the rays, lane 0 runs the controller
// One wavefront per instance, lane l takes the rays l, l + 64, ..., the same tree sum and the same controller as the box kernels: all of it is
// range_device.hpp's one body.  What is new is per-lane and data-dependent: every lane walks the skip-link hierarchy of mesh_bvh.hpp on its
// own, forward only, so there is no stack, no LDS and no scratch.  Node (64 B) and triangle (72 B) fetches are per-lane global loads; the rays
// of a region of interest span a few degrees, so the lanes of a wave mostly walk the same nodes and share their cache lines.  FP64.
#include <hip/hip_runtime.h>

#include "range_device.hpp"

#pragma clang fp contract(off)

namespace brov {

// 256 threads = 4 wavefronts = 4 instances per block, as the box kernels
__global__ __launch_bounds__(256) void mesh_eval_kernel(brov_range_params P, RangeScene S, MeshDev M, const double* __restrict__ sigma, int B, int m,
                                                        const double* __restrict__ x, double* __restrict__ range, int32_t* __restrict__ hits,
                                                        double* __restrict__ rot, double* __restrict__ depth, long long* __restrict__ visits) {
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
    if (b >= B) return;
    double r;
    int n;
    range_wave_on<true>(P, S, M, sigma, b, m, lane, x + (size_t)b * 12, rot, depth, r, n, visits ? visits + (size_t)b * 2 : nullptr);
    if (lane == 0) { range[b] = r; hits[b] = n; }
}

__global__ __launch_bounds__(256) void inspect_mesh_tick_kernel(brov_range_params P, RangeScene S, MeshDev M, const double* __restrict__ sigma,
                                                                brov_inspect_params C, InspectDev D, int B, int m, const double* __restrict__ x,
                                                                const double* __restrict__ y, brov_result* __restrict__ res) {
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
    if (b >= B) return;
    double r;
    int n;
    range_wave_on<true>(P, S, M, sigma, b, m, lane, x + (size_t)b * 12, nullptr, nullptr, r, n, nullptr);
    if (lane != 0) return;
    inspect_tick_lane0(C, D, b, r, y, res);
}

void launch_mesh_eval(const brov_range_params& P, const RangeScene& S, const MeshDev& M, const double* sigma, int B, long long m, const double* x,
                      double* range, int32_t* hits, double* rot, double* depth, long long* visits, hipStream_t st) {
    hipLaunchKernelGGL(mesh_eval_kernel, dim3((B + 3) / 4), dim3(256), 0, st, P, S, M, sigma, B, (int)m, x, range, hits, rot, depth, visits);
}
void launch_inspect_mesh_tick(const brov_range_params& P, const RangeScene& S, const MeshDev& M, const double* sigma, const brov_inspect_params& C,
                              const InspectDev& D, int B, long long m, const double* x, const double* y, brov_result* res, hipStream_t st) {
    hipLaunchKernelGGL(inspect_mesh_tick_kernel, dim3((B + 3) / 4), dim3(256), 0, st, P, S, M, sigma, C, D, B, (int)m, x, y, res);
}

}  // namespace brov
