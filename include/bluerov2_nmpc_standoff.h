/* bluerov2_nmpc_standoff.h -- brov_standoff_*: the stand-off term of the fleet planning loop.  The fleet picks each
 * vehicle's cheapest candidate; since the clearance term (brov_clearance_*) a candidate is priced by its closest approach to the OTHER
 * VEHICLES' plans.  This term prices it by its closest approach to the STRUCTURE: the scene of the solver's range stage, that is the boxes of
 * brov_range_set_scene_host and the triangle mesh of brov_mesh_set_host, as they stand when a step is launched (the range stage itself need
 * not be on).  Sampling-based avoidance over the solver's candidates: nothing enters the solver's own problem.  Part of the C ABI of
 * bluerov2_nmpc.h, which includes this file behind bluerov2_nmpc_mesh.h; not meant to be included on its own.  These calls take a
 * brov_fleet; brov_fleet_last_error() has their texts, each of which begins with the call's name.
 *
 * The rules (tests/standoff_restatement.py restates them in numpy and is held byte for byte).  Every product, sum, difference and quotient
 * is rounded once; a dot product is  rn(rn(rn(a_x b_x) + rn(a_y b_y)) + rn(a_z b_z));  a triangle is the stored form (v0, e1, e2) of the mesh.
 *
 * Point and triangle.  For a point p:
 *     a = p - v0,  b = a - e1,  c = a - e2                                   (componentwise)
 *     d1 = e1.a, d2 = e2.a, d3 = e1.b, d4 = e2.b, d5 = e1.c, d6 = e2.c
 *     vc = d1 d4 - d3 d2,  vb = d5 d2 - d1 d6,  va = d3 d6 - d5 d4
 *     (s, t) = the first rule that holds:
 *       1  d1 <= 0 and d2 <= 0                                    (0, 0)
 *       2  d3 >= 0 and d4 <= d3                                   (1, 0)
 *       3  vc <= 0 and d1 >= 0 and d3 <= 0                        (d1 / (d1 - d3), 0)
 *       4  d6 >= 0 and d5 <= d6                                   (0, 1)
 *       5  vb <= 0 and d2 >= 0 and d6 <= 0                        (0, d2 / (d2 - d6))
 *       6  va <= 0 and g = d4 - d3 >= 0 and h = d5 - d6 >= 0      w = g / (g + h);  (1 - w, w)
 *       7  otherwise                                              den = 1 / ((va + vb) + vc);  (vb den, vc den)
 *     r_c = (a_c - s e1_c) - t e2_c;   D2 = r.r
 * (the closest point of the triangle by its Voronoi regions).  A degenerate stored triangle (e1 = e2 = 0) has no special case: rule 1 makes
 * it the point v0.
 * Point and box [lo, hi]:  e_c = max(max(lo_c - p_c, p_c - hi_c), 0),  D2 = (e_x^2 + e_y^2) + e_z^2;  0 inside the box.
 *
 * A candidate's value, b = v * C + c:  s2[b] = min(reach2, min D2)  over the stages k = first ... N of the solver's iterate x[b][k][0..2], all
 * triangles and all boxes.  The minimum starts at reach2 = reach * reach (formed once on the host; reach = +Inf is allowed) and is updated by
 * D2 < m, so a NaN D2 is skipped; a stage with a NaN coordinate is skipped outright.  Two calls return the same bytes, and the bytes depend
 * neither on the launch geometry nor on the mesh's leaf size.  The hierarchy of the mesh is walked with the running minimum as its bound, so
 * a finite reach is what makes the term cheap: nothing farther than reach is ever looked at closely, and nothing farther than that can
 * matter to a re-score as long as reach >= radius.
 *
 * Re-score: the clearance term's rule on s2.  cost := cost + weight * (r2 - s2[b]) where s2[b] < r2 = radius * radius, the same three rounded
 * operations; a cost that is NaN already keeps its bytes, a NaN the sum generates is written as the quiet NaN 0x7ff8000000000000; weight = +Inf
 * makes the candidate ineligible.  With the clearance term on as well, clearance re-scores first and this term re-scores the records that
 * come out of it.
 *
 * first: stage 0 is the vehicle's own position and is shared by all its candidates.  Under a hard weight and first = 0 a vehicle already inside
 * the radius has no eligible candidate and holds its input for ever; hence first = 1 is what the Python mirror defaults to.
 *
 * Statistics per vehicle, reset where the clearance term's are (brov_fleet_reset, brov_fleet_set_state_host): last_s2, s2 of the step's winner
 * or -1.0 without one; min_s2, its minimum over the steps that had a winner, +Inf before the first; below, the number of steps whose winner
 * had s2 < r2.
 *
 * The scene is read per step.  brov_range_set_scene_host and brov_mesh_set_host wait for the whole device before they change or free
 * anything, so a step in flight on any stream keeps the mesh it was launched with and the next step sees the new one; the caller owes no
 * wait.  With the term off (the default, and after brov_standoff_off) every call launches exactly what it launched before. */
#ifndef BLUEROV2_NMPC_STANDOFF_H_
#define BLUEROV2_NMPC_STANDOFF_H_
#ifndef BLUEROV2_NMPC_H_
#error "include bluerov2_nmpc.h, which includes this file"
#endif

/* turns the term on.  BROV_ERR_ARG unless: radius finite and > 0 with a finite square > 0, weight > 0 (+Inf allowed), reach >= radius (+Inf
 * allowed, NaN not), 0 <= first <= N, and the solver's scene holds a box or a mesh.  brov_fleet_step and the closed loops are refused, with their
 * own name in the text, while the term is on and the scene has been emptied since */
int brov_standoff_set(brov_fleet* f, double radius, double weight, double reach, int first);
int brov_standoff_off(brov_fleet* f);                                  /* the parameters and the statistics are kept */
int brov_standoff_enabled(const brov_fleet* f);                        /* 0 for NULL */
/* the kernels alone against the scene as it stands; they move nothing.  x DEVICE [B][N+1][12] (NULL: the solver's iterate), rec DEVICE [B]
 * (NULL: the solver's records), s2 DEVICE [B], out DEVICE [B] the re-scored records or NULL, visits DEVICE [B][2] or NULL: the node tests and
 * the triangle tests the walks of each candidate made.  Ordered behind the solver's last stream and the fleet's own last work.  Refused while
 * the term is off */
int brov_standoff_eval_device(brov_fleet* f, const double* x, const brov_result* rec, double* s2, brov_result* out, int64_t* visits, void* stream);
int brov_standoff_eval_host(brov_fleet* f, const brov_result* rec_host /*[B] or NULL*/, double* s2 /*[B]*/, brov_result* out /*[B] or NULL*/,
                            int64_t* visits /*[B][2] or NULL*/);
int brov_standoff_get_stats_host(brov_fleet* f, double* last_s2, double* min_s2, int32_t* below /*[V] each, any NULL*/);
int brov_standoff_last_seconds(brov_fleet* f, double* seconds);        /* the distance kernel, HIP events */

#endif
