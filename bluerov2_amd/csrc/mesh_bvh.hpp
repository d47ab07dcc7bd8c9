// mesh_bvh.hpp -- the host-side builder of the range stage's mesh (brov_mesh_*, include/bluerov2_nmpc_mesh.h): the triangles as the device
// reads them (v0, e1, e2) and a skip-link ("threaded") bounding-volume hierarchy over them.  Median split of the triangle centroids along
// their widest axis with a stable sort, leaves of at most `leaf` triangles, nodes in depth-first order; every node carries the index to go to
// on a miss or after a leaf, so a traversal is one forward walk  i = hit && interior ? i + 1 : skip  that ends at i == nodes: no stack, hence
// no scratch and no LDS on the device.  The node boxes are padded by 2^-30 x the mesh's largest extent (DESIGN.md section 4.9k argues why
// that makes the culling conservative).  The structure's only contract is that a traversal gives the result of testing every triangle.
// Plain C++17: no HIP, no device; tests/mesh_bvh_main.cpp compiles it alone under the address and undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

namespace brov {

struct MeshNode {                 // 64 bytes
    double lo[3], hi[3];          // the padded box of the subtree
    int32_t skip;                 // where to go on a miss, and after a leaf
    int32_t first, count;         // a leaf's triangles [first, first + count) in leaf order; count == 0: an interior node
    int32_t reserved_;
};
struct MeshTri { double v0[3], e1[3], e2[3]; };   // 72 bytes
static_assert(sizeof(MeshNode) == 64 && sizeof(MeshTri) == 72, "the device layout");

struct MeshBvh {
    std::vector<MeshNode> nodes;
    std::vector<MeshTri> tris;        // in leaf order
    std::vector<int32_t> order;       // tris[k] is the caller's triangle order[k]
    double pad = 0.0;
    int32_t depth = 0, leaves = 0, leaf = 0;
};

// the stored form of one triangle t [3][3]: each edge component one rounded subtraction; a triangle whose rounded cross product e1 x e2 is
// zero gets e1 = e2 = 0 (det == 0 for every ray: never hit)
inline MeshTri mesh_stored_triangle(const double* t) {
    MeshTri r;
    for (int c = 0; c < 3; c++) {
        r.v0[c] = t[c];
        r.e1[c] = t[3 + c] - t[c];
        r.e2[c] = t[6 + c] - t[c];
    }
    bool zero = true;
    for (int c = 0; c < 3; c++) {
        const int a = (c + 1) % 3, b = (c + 2) % 3;
        // (volatile: two separately rounded products, whatever the host compiler's contraction default)
        volatile double p1 = r.e1[a] * r.e2[b], p2 = r.e1[b] * r.e2[a];
        if (p1 - p2 != 0.0) zero = false;
    }
    if (zero)
        for (int c = 0; c < 3; c++) r.e1[c] = r.e2[c] = 0.0;
    return r;
}

namespace mesh_detail {
struct Builder {
    const double* tri;
    int leaf;
    MeshBvh& out;
    std::vector<double> cen;   // [n][3] three times the centroid: the vertex sum
    void bounds(int a, int b, double (&lo)[3], double (&hi)[3]) const {
        for (int c = 0; c < 3; c++) { lo[c] = HUGE_VAL; hi[c] = -HUGE_VAL; }
        for (int k = a; k < b; k++) {
            const double* t = tri + (size_t)out.order[k] * 9;
            for (int v = 0; v < 3; v++)
                for (int c = 0; c < 3; c++) { lo[c] = std::min(lo[c], t[v * 3 + c]); hi[c] = std::max(hi[c], t[v * 3 + c]); }
        }
    }
    void build(int a, int b, int depth) {
        const int idx = (int)out.nodes.size();
        out.nodes.push_back(MeshNode{});
        double lo[3], hi[3];
        bounds(a, b, lo, hi);
        for (int c = 0; c < 3; c++) { out.nodes[idx].lo[c] = lo[c] - out.pad; out.nodes[idx].hi[c] = hi[c] + out.pad; }
        out.depth = std::max(out.depth, depth);
        if (b - a <= leaf) {
            out.nodes[idx].first = a;
            out.nodes[idx].count = b - a;
            out.nodes[idx].skip = idx + 1;
            out.leaves++;
            return;
        }
        double clo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, chi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
        for (int k = a; k < b; k++)
            for (int c = 0; c < 3; c++) {
                const double v = cen[(size_t)out.order[k] * 3 + c];
                clo[c] = std::min(clo[c], v); chi[c] = std::max(chi[c], v);
            }
        int axis = 0;
        for (int c = 1; c < 3; c++)
            if (chi[c] - clo[c] > chi[axis] - clo[axis]) axis = c;
        std::stable_sort(out.order.begin() + a, out.order.begin() + b,
                         [&](int32_t p, int32_t q) { return cen[(size_t)p * 3 + axis] < cen[(size_t)q * 3 + axis]; });
        const int mid = a + (b - a) / 2;   // by position: identical centroids split as well
        build(a, mid, depth + 1);
        build(mid, b, depth + 1);
        out.nodes[idx].skip = (int)out.nodes.size();
    }
};
}  // namespace mesh_detail

// the structure over n >= 1 triangles tri [n][3][3] with finite coordinates, leaves of at most leaf >= 1 triangles
inline void mesh_bvh_build(int64_t n, const double* tri, int leaf, MeshBvh& out) {
    out = MeshBvh{};
    out.leaf = leaf;
    out.order.resize((size_t)n);
    std::iota(out.order.begin(), out.order.end(), 0);
    mesh_detail::Builder bd{tri, leaf, out, std::vector<double>((size_t)n * 3)};
    for (int64_t k = 0; k < n; k++)
        for (int c = 0; c < 3; c++) bd.cen[(size_t)k * 3 + c] = (tri[k * 9 + c] + tri[k * 9 + 3 + c]) + tri[k * 9 + 6 + c];
    double lo[3], hi[3];
    bd.bounds(0, (int)n, lo, hi);
    out.pad = std::ldexp(std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2])), -30);
    out.nodes.reserve((size_t)(2 * n));
    bd.build(0, (int)n, 0);
    out.tris.resize((size_t)n);
    for (int64_t k = 0; k < n; k++) out.tris[(size_t)k] = mesh_stored_triangle(tri + (size_t)out.order[(size_t)k] * 9);
}

}  // namespace brov
