// standoff_kernel.hpp -- launchers of the stand-off kernels (standoff_kernel.hip) for their host side (fleet_api.hip, brov_standoff_*), and the
// one thing that host side asks of the solver beyond its public calls: the scene of the range stage as it stands on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_device.hpp"
#include "nmpc_device.hpp"

namespace brov {

// the boxes of brov_range_set_scene_host and the mesh of brov_mesh_set_host as the solver's own kernels are handed them; filled by
// nmpc_api.hip.  The mesh's two device blocks are freed by brov_mesh_set_host behind a wait for the whole device, never under a launch
struct SceneView {
    RangeScene boxes{};
    MeshDev mesh;
    bool empty() const { return boxes.n < 1 && mesh.n_tris < 1; }
};
SceneView solver_scene(const brov_solver* s);

// how many grid-level slices the stages first ... N are cut into when every slice holds `per` stages
inline int standoff_slices(int N, int first, int per) { return (N + 1 - first + per - 1) / per; }

// part[s][b] = min(reach2, min over the stages k of slice s, the boxes of S and the triangles of M of D2(x[b][k][0..2])), s = 0 ...
// standoff_slices(N, first, per) - 1, slice s holding the stages first + s * per ... min(first + (s + 1) * per - 1, N); a stage with a NaN
// coordinate is skipped.  x DEVICE [B][N+1][12], part DEVICE [slices][B].  visits (or nullptr; needs per >= N + 1 - first: one slice):
// DEVICE [B][2] node tests and triangle tests per candidate
void launch_standoff_dist(const double* x, const RangeScene& S, const MeshDev& M, int B, int N, int first, int per, double reach2, double* part,
                          long long* visits, hipStream_t st);

// behind the select: last_s2[v] = s2 of the winner or -1, min_s2[v] its running minimum over the steps with a winner, below[v] += s2 < r2
void launch_standoff_stats(const int32_t* winner, const double* s2, int V, int C, double r2, double* last_s2, double* min_s2, int32_t* below,
                           hipStream_t st);

}  // namespace brov
