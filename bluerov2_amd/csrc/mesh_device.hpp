// mesh_device.hpp -- what the host side and the kernels of the range stage's mesh agree on (mesh_kernel.hip; include/bluerov2_nmpc_mesh.h,
// brov_mesh_*): the structure on the device as the kernel arguments carry it, and the two launchers.
#pragma once
#include <hip/hip_runtime.h>

#include "nmpc_device.hpp"
#include "mesh_bvh.hpp"

namespace brov {

struct MeshDev {                  // shared by the batch: the pointers and counts are wave-uniform, the nodes and triangles per-lane global loads
    const MeshNode* nodes = nullptr;   // [n_nodes] in depth-first order (mesh_bvh.hpp)
    const MeshTri* tris = nullptr;     // [n_tris] in leaf order
    int32_t n_nodes = 0, n_tris = 0;
};
// launch_range_eval with the mesh M beside the boxes; visits [B][2] node tests and triangle tests per instance, or nullptr
void launch_mesh_eval(const brov_range_params& P, const RangeScene& S, const MeshDev& M, const double* sigma, int B, long long m, const double* x,
                      double* range, int32_t* hits, double* rot, double* depth, long long* visits, hipStream_t st);
// launch_inspect_tick with the mesh M beside the boxes
void launch_inspect_mesh_tick(const brov_range_params& P, const RangeScene& S, const MeshDev& M, const double* sigma, const brov_inspect_params& C,
                              const InspectDev& D, int B, long long m, const double* x, const double* y, brov_result* res, hipStream_t st);

}  // namespace brov
