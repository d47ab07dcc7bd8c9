// standoff_walk.hpp -- the arithmetic of the fleet loop's stand-off term (include/bluerov2_nmpc_standoff.h, brov_standoff_*; DESIGN.md section
// 4.12d; the specification is tests/standoff_restatement.py): the squared distance of a point from a box and from a stored triangle of
// mesh_bvh.hpp, and the nearest-distance walk over its skip-link hierarchy.  One body for the device (standoff_kernel.hip) and for the host:
// tests/standoff_walk_main.cpp compiles this file alone, without HIP, under the address and undefined-behaviour sanitizers and holds the
// walk to brute force.  Every product, sum, difference and quotient is rounded once: clang compiles what follows with contraction off
// (the instructions carry no contract flag wherever they are inlined), any other compiler is given -ffp-contract=off.
#pragma once
#include <cstdint>

#include "mesh_bvh.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BROV_STANDOFF_FN __host__ __device__ __forceinline__
#else
#define BROV_STANDOFF_FN inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace brov {

// a node is culled iff slack x (squared distance from its padded box) > the running minimum: section 4.12d argues why that never culls a
// triangle that would have lowered the minimum
constexpr double kStandoffSlack = 1.0 - 0x1.0p-20;

// the larger of two numbers neither of which is NaN (the callers skip NaN points; the bounds of boxes and nodes are finite)
BROV_STANDOFF_FN double standoff_max(double x, double y) { return x > y ? x : y; }

// the squared distance of p from the box [lo, hi]: e_c = max(max(lo_c - p_c, p_c - hi_c), 0), (e_x^2 + e_y^2) + e_z^2; 0 inside
BROV_STANDOFF_FN double standoff_box_d2(const double (&p)[3], const double* lo, const double* hi) {
    const double ex = standoff_max(standoff_max(lo[0] - p[0], p[0] - hi[0]), 0.0);
    const double ey = standoff_max(standoff_max(lo[1] - p[1], p[1] - hi[1]), 0.0);
    const double ez = standoff_max(standoff_max(lo[2] - p[2], p[2] - hi[2]), 0.0);
    return (ex * ex + ey * ey) + ez * ez;
}

BROV_STANDOFF_FN double standoff_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the squared distance of p from the stored triangle (v0, e1, e2): the closest point v0 + s e1 + t e2 by its Voronoi region, the first rule
// that holds (bluerov2_nmpc_standoff.h numbers them).  Each rule has at most one quotient, so one division serves all seven: the operands
// are selected, the quotient is the rule's own.  A degenerate stored triangle (e1 = e2 = 0) falls under rule 1: the point v0.  Every
// comparison is false on a NaN; what comes out then is NaN or Inf and never lowers a minimum
BROV_STANDOFF_FN double standoff_tri_d2(const double (&p)[3], const MeshTri& T) {
    double a[3], b[3], c[3], e1[3], e2[3];
    for (int j = 0; j < 3; j++) {
        e1[j] = T.e1[j]; e2[j] = T.e2[j];
        a[j] = p[j] - T.v0[j];
        b[j] = a[j] - e1[j];
        c[j] = a[j] - e2[j];
    }
    const double d1 = standoff_dot(e1, a), d2 = standoff_dot(e2, a), d3 = standoff_dot(e1, b), d4 = standoff_dot(e2, b);
    const double d5 = standoff_dot(e1, c), d6 = standoff_dot(e2, c);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double g = d4 - d3, h = d5 - d6;
    int rule;
    double num = 0.0, den = 1.0;
    if (d1 <= 0.0 && d2 <= 0.0) rule = 1;
    else if (d3 >= 0.0 && d4 <= d3) rule = 2;
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { rule = 3; num = d1; den = d1 - d3; }
    else if (d6 >= 0.0 && d5 <= d6) rule = 4;
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { rule = 5; num = d2; den = d2 - d6; }
    else if (va <= 0.0 && g >= 0.0 && h >= 0.0) { rule = 6; num = g; den = g + h; }
    else { rule = 7; num = 1.0; den = (va + vb) + vc; }
    const double q = num / den;
    const double s = rule == 2 ? 1.0 : rule == 3 ? q : rule == 6 ? 1.0 - q : rule == 7 ? vb * q : 0.0;
    const double t = rule == 4 ? 1.0 : rule == 5 || rule == 6 ? q : rule == 7 ? vc * q : 0.0;
    double r[3];
    for (int j = 0; j < 3; j++) r[j] = (a[j] - s * e1[j]) - t * e2[j];
    return standoff_dot(r, r);
}

// m := the lower of m and the squared distance of p (no NaN coordinate) from the nearest of the triangles, by a forward walk over the nodes
// in depth-first order: a culled node and a leaf go on at their skip link, an interior node at the next index.  No stack.  nt, tt: the node
// tests and triangle tests made
BROV_STANDOFF_FN double standoff_mesh_walk(const MeshNode* nodes, int32_t n_nodes, const MeshTri* tris, const double (&p)[3], double m, int& nt, int& tt) {
    int32_t i = 0;
    while (i < n_nodes) {
        const MeshNode& nd = nodes[i];
        const double lb = standoff_box_d2(p, nd.lo, nd.hi) * kStandoffSlack;
        const int32_t skip = nd.skip, first = nd.first, count = nd.count;
        nt++;
        if (lb > m) { i = skip; continue; }
        for (int32_t k = first; k < first + count; k++) {
            const double d = standoff_tri_d2(p, tris[k]);
            tt++;
            if (d < m) m = d;   // a NaN distance compares false: skipped
        }
        i = count > 0 ? skip : i + 1;
    }
    return m;
}

// the same minimum by testing every triangle: what the walk is held to
BROV_STANDOFF_FN double standoff_mesh_brute(const MeshTri* tris, int32_t n_tris, const double (&p)[3], double m) {
    for (int32_t k = 0; k < n_tris; k++) {
        const double d = standoff_tri_d2(p, tris[k]);
        if (d < m) m = d;
    }
    return m;
}

}  // namespace brov

#undef BROV_STANDOFF_FN
