// standoff_kernel.hip -- the stand-off term of the fleet planning loop (include/bluerov2_nmpc_standoff.h, brov_standoff_*; DESIGN.md section
// 4.12d; the specification is tests/standoff_restatement.py).  Behind a solve, ahead of the fleet's select:
//   standoff_dist_kernel    per candidate b = v * C + c and slice of the stages first ... N the squared distance of closest approach of its
//                           predicted path x[b][k][0..2] to the solver's scene -- the boxes and the triangle mesh of the range stage --, capped
//                           at reach2; clearance_rescore_kernel (clearance_kernel.hip) folds the slices and re-scores the records: its
//                           part[slice][b] layout and its rule are exactly these
// and behind the select:
//   standoff_stats_kernel   the step's statistics from the winners
//
// standoff_dist_kernel: lane <-> candidate, the stages on blockIdx.y, one wavefront per block.  The 64 lanes of a wavefront hold 64
// consecutive candidates at the SAME stage: the candidates of a vehicle leave from one state, so the lanes mostly walk the same nodes and share
// their cache lines, and the store part[slice][b] is coalesced.  Per query point the boxes come first: the scene travels by value in the kernel
// arguments, its bounds are wave-uniform and read through the scalar cache.  Then the forward walk over the skip-link hierarchy of mesh_bvh.hpp,
// mesh_ray's shape: per-lane global loads of 64-byte nodes and 72-byte triangles, one index, no stack, no LDS, no scratch.  The running
// minimum starts at reach2, which is what culls (section 4.12d has the counts).  No atomics: a minimum of non-NaN, never -0.0 values does not
// depend on the order it is taken in, so the bytes depend neither on the launch geometry nor on the leaf size, and two calls return the same
// bytes.  The arithmetic is standoff_walk.hpp's, every operation rounded on its own.  FP64.
#include <hip/hip_runtime.h>

#include "standoff_kernel.hpp"
#include "standoff_walk.hpp"

#pragma clang fp contract(off)

namespace brov {

constexpr int kStandoffNX = 12;   // doubles per stage of the iterate

__global__ __launch_bounds__(64) void standoff_dist_kernel(const double* __restrict__ x, RangeScene S, MeshDev M, int B, int N, int first, int per,
                                                           double reach2, double* __restrict__ part, long long* __restrict__ visits) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;   // (no barrier below)
    const int k0 = first + (int)blockIdx.y * per;
    const int k1 = k0 + per - 1 < N ? k0 + per - 1 : N;
    const double* __restrict__ xs = x + (size_t)b * (N + 1) * kStandoffNX;
    const int nbox = S.n;
    double m = reach2;
    int nt = 0, tt = 0;
    for (int k = k0; k <= k1; k++) {
        const double p[3] = {xs[(size_t)k * kStandoffNX + 0], xs[(size_t)k * kStandoffNX + 1], xs[(size_t)k * kStandoffNX + 2]};
        if (p[0] != p[0] || p[1] != p[1] || p[2] != p[2]) continue;   // a stage that is not a number is no point of the path
        for (int j = 0; j < nbox; j++) {
            const double d = standoff_box_d2(p, S.lo[j], S.hi[j]);
            if (d < m) m = d;
        }
        m = standoff_mesh_walk(M.nodes, M.n_nodes, M.tris, p, m, nt, tt);
    }
    part[(size_t)blockIdx.y * B + b] = m;
    if (visits) {   // (the host launches one slice: the lane has walked all stages of its candidate)
        visits[(size_t)b * 2 + 0] = nt;
        visits[(size_t)b * 2 + 1] = tt;
    }
}

// one thread per vehicle
__global__ __launch_bounds__(128) void standoff_stats_kernel(const int32_t* __restrict__ winner, const double* __restrict__ s2, int V, int C, double r2,
                                                             double* __restrict__ last_s2, double* __restrict__ min_s2, int32_t* __restrict__ below) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int win = winner[v];
    if (win >= 0) {
        const double d = s2[(size_t)v * C + win];
        last_s2[v] = d;
        if (d < min_s2[v]) min_s2[v] = d;
        if (d < r2) below[v] += 1;
    } else {
        last_s2[v] = -1.0;
    }
}

void launch_standoff_dist(const double* x, const RangeScene& S, const MeshDev& M, int B, int N, int first, int per, double reach2, double* part,
                          long long* visits, hipStream_t st) {
    hipLaunchKernelGGL(standoff_dist_kernel, dim3((unsigned)((B + 63) / 64), (unsigned)standoff_slices(N, first, per)), dim3(64), 0, st, x, S, M, B, N,
                       first, per, reach2, part, visits);
}
void launch_standoff_stats(const int32_t* winner, const double* s2, int V, int C, double r2, double* last_s2, double* min_s2, int32_t* below,
                           hipStream_t st) {
    hipLaunchKernelGGL(standoff_stats_kernel, dim3((unsigned)((V + 127) / 128)), dim3(128), 0, st, winner, s2, V, C, r2, last_s2, min_s2, below);
}

}  // namespace brov
