/* bluerov2_nmpc_mesh.h -- brov_mesh_*: triangle meshes in the scene of the range stage.  The reference's bridge demo does not fly against
 * boxes: start_bridge_demo spawns bluerov2_environ/urdf/bridge2.urdf, whose visual and collision geometry is meshes/bridge2.STL under the
 * origin rpy = (pi/2, 0, 0).  A mesh is a list of WORLD-frame triangles, shared by the batch, that lives beside the boxes of
 * brov_range_set_scene_host: a ray's depth is the smallest over both.  Part of the C ABI of bluerov2_nmpc.h, which includes this file behind
 * bluerov2_nmpc_curve.h; not meant to be included on its own.
 *
 * The ray-triangle test.  The ray is the range stage's own (bluerov2_nmpc_inspect.h): origin o = p + Rot mount, direction D = Rot (1, -a, -b),
 * so the ray parameter t is the depth.  Per triangle (v0, v1, v2) the HOST stores v0, e1 = v1 - v0 and e2 = v2 - v0, each component one
 * rounded double subtraction.  A triangle whose rounded cross product e1 x e2 (below) is zero in all three components is DEGENERATE: it is
 * stored with e1 = e2 = 0, so that its det is exactly 0 and it is never hit.  On the device every product, sum and quotient is rounded once;
 * a cross product is  (a x b)_x = rn(rn(a_y b_z) - rn(a_z b_y))  and cyclic, a dot product  rn(rn(rn(a_x b_x) + rn(a_y b_y)) + rn(a_z b_z)):
 *   p = D x e2;   det = e1 . p;   inv = 1 / det (the IEEE quotient);   s = o - v0
 *   u = (s . p) inv;   q = s x e1;   v = (D . q) inv;   t = (e2 . q) inv
 * (the Moeller-Trumbore test).  A hit requires all of  det != 0,  u >= 0,  v >= 0,  rn(u + v) <= 1,  t >= near  and  t <= far.  Both faces
 * count.  Every comparison is false on a NaN, so a NaN anywhere is a miss.  The ray's depth is the smallest hit t over the triangles and the
 * smallest hit tn over the boxes; range, mean, tree sum, noise and the no-return value 0.0 are those of the box stage.  A numpy restatement
 * given the same Rot agrees per ray bit for bit (tests/mesh_restatement.py: brute force over all triangles).  The test is not watertight: a
 * ray through a shared edge may in principle miss both neighbours.
 *
 * The acceleration structure is internal (a skip-link bounding-volume hierarchy built on the host, bluerov2_amd/csrc/mesh_bvh.hpp); its only
 * contract is that THE RESULT IS THAT OF TESTING EVERY TRIANGLE.  `leaf` sets the largest number of triangles in a leaf and changes no bit of
 * any result.  brov_mesh_summary reports its shape.
 * With no mesh set, and after brov_mesh_set_host(s, 0, ...), every launch is the one of a solver that never touched this API. */
#ifndef BLUEROV2_NMPC_MESH_H_
#define BLUEROV2_NMPC_MESH_H_
#ifndef BLUEROV2_NMPC_H_
#error "include bluerov2_nmpc.h, which includes this file"
#endif

#define BROV_MESH_MAX_TRIANGLES 1048576
#define BROV_MESH_DEFAULT_LEAF 4
#define BROV_MESH_MAX_LEAF 8
typedef struct brov_mesh_summary {
    int64_t triangles;
    int64_t nodes;
    int64_t leaves;
    int64_t device_bytes;  /* nodes (64 B each) and triangles (72 B each) */
    double pad;            /* the node boxes are wider than their triangles by this on every side: 2^-30 x the mesh's largest extent */
    int32_t depth;         /* edges from the root to the deepest leaf */
    int32_t leaf;          /* the leaf size in force, 1 ... BROV_MESH_MAX_LEAF; 0 with no mesh */
} brov_mesh_summary;

/* the mesh: n triangles, tri [n][3][3] (triangle, vertex, xyz) in the world frame; leaf 0: BROV_MESH_DEFAULT_LEAF.  n = 0 removes the mesh
 * (tri may be NULL).  Refused with BROV_ERR_ARG and a text in brov_last_error() that starts with the call's name, before anything is waited
 * for or allocated: n outside 0 ... BROV_MESH_MAX_TRIANGLES, a NULL tri with n > 0, a non-finite coordinate, leaf outside
 * 0 ... BROV_MESH_MAX_LEAF.  Degenerate triangles are accepted and never hit */
int brov_mesh_set_host(brov_solver* s, int64_t n, const double* tri, int32_t leaf);
/* the mesh in force; all zeros with none */
int brov_mesh_info(brov_solver* s, brov_mesh_summary* info);
/* brov_range_eval_host (same arguments, same contract; it casts against the mesh as well, as every caster does once a mesh is set), and
 * per instance the number of node-box tests and of triangle tests its rays made: visits [b][0], [b][1].  Refused without a mesh */
int brov_mesh_eval_host(brov_solver* s, int64_t m, const double* x /*[B][12]*/, double* range /*[B]*/, int32_t* hits /*[B]*/,
                        double* rot /*[B][9] or NULL*/, double* depth /*[B][roi * roi] or NULL*/, int64_t* visits /*[B][2] or NULL*/);

#endif
